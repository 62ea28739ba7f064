"""From files at device rate: cv.imread of the reference's input pipeline (apps/eval.py:56,
dataset/interhand.py:223 over dataset/prepare_data.py:123-166's <split>/img/<idx>.jpg) split in two.

    host   (decode worker processes, lib/libdir_jpeg.so, include/dir_jpeg.h)   the Huffman stream -> one RECORD per image: a 512-byte header + the
                                                                               quantised DCT coefficients (int16) -- the only inherently serial part
    GPU    (dir_jpeg_decode_records, csrc/jpeg.hip)                            dequantise + integer IDCT + chroma upsampling + YCbCr -> BGR uint8
                                                                               [B,256,256,3]: what the stem kernel reads

bit-exact with libjpeg(-turbo), the decoder OpenCV and Pillow both use (oracle/jpeg.py is pinned to Pillow's).  A 4:2:0 record has the size of
the decoded frame, so the host -> device traffic is unchanged while the host's work per image falls to the entropy decode (PIL's full decode was
what saturated the 16-CPU quota at 22 k images/s, profiles/r04_fromdisk_sweep_flag_ring.txt).  Files the entropy decoder refuses (progressive,
arithmetic, CMYK) or that are not 256x256 are decoded the ordinary way on the host (dataset.decode_bgr) and travel as PIXEL records.

The ENCODE path is the mirror image (cv.imwrite of dataset/prepare_data.py:174-214, the mask/ and dense/ frames):

    GPU    (dir_jpeg_encode_records, csrc/jpeg_enc.hip)                        uint8 frames [B,H,W,3] -> colour conversion, 4:2:0 downsampling, integer
                                                                               forward DCT, quantisation -> one record per frame (RecordEncoder)
    host   (dir_jpeg_encode_record, include/dir_jpeg_enc.h)                    record -> Huffman coding + file syntax (record_to_bytes, write_record)

and the file equals the one libjpeg(-turbo) writes for the frame at the same quality, byte for byte (tests/test_jpeg_enc_ref.py,
tests/test_gpu_jpeg_enc.py).  jpeg_round_trip: encode then decode on the device = the pixels cv.imread gives back from such a file.

Plumbing only: pointers, sizes, error codes.  No GPU call happens in a worker process (libdir_jpeg.so has no GPU runtime in it)."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _capi

HEADER_BYTES = 512
MAGIC, MAGIC_PIXELS = 0x4a524944, 0x50524944
_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.environ.get('DIR_JPEG_LIB_PATH') or os.path.join(os.path.dirname(_HERE), 'lib', 'libdir_jpeg.so')
_host = None


def host_lib():
    """libdir_jpeg.so (built by dir_amd/build.py with gcc).  No fallback: a missing library is an error."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise _capi.DirHipError('%s not found: run python -m dir_amd.build' % HOST_LIB_PATH)
        lib = C.CDLL(HOST_LIB_PATH)
        lib.dir_jpeg_decode_coefficients.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.dir_jpeg_decode_coefficients.restype = C.c_int
        lib.dir_jpeg_record_bytes.argtypes = [C.c_int] * 5
        lib.dir_jpeg_record_bytes.restype = C.c_size_t
        lib.dir_jpeg_abi_version.restype = C.c_int
        if lib.dir_jpeg_abi_version() != 1:
            raise _capi.DirHipError('libdir_jpeg.so ABI version %d != 1' % lib.dir_jpeg_abi_version())
        lib.dir_jpeg_encode_record.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.dir_jpeg_encode_record.restype = C.c_int
        lib.dir_jpeg_encode_bound.argtypes = [C.c_void_p, C.c_size_t]
        lib.dir_jpeg_encode_bound.restype = C.c_size_t
        lib.dir_jpeg_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        lib.dir_jpeg_quality_tables.restype = C.c_int
        lib.dir_jpeg_enc_abi_version.restype = C.c_int
        if lib.dir_jpeg_enc_abi_version() != 1:
            raise _capi.DirHipError('libdir_jpeg.so encoder ABI version %d != 1' % lib.dir_jpeg_enc_abi_version())
        _host = lib
    return _host


def record_bytes(size=256, hsamp=2, vsamp=2, ncomp=3):
    """bytes of one record of a size x size image with these luma sampling factors (4:2:0 = the default of cv.imwrite / libjpeg), a multiple of 16"""
    n = int(host_lib().dir_jpeg_record_bytes(size, size, hsamp, vsamp, ncomp))
    assert n > 0
    return (n + 15) // 16 * 16


def file_to_record(path, row, size=256):
    """one file -> `row` (a contiguous uint8 numpy array of record size).  Baseline size x size JPEGs become coefficient records; anything else is
    decoded on the host (dataset.decode_bgr: libjpeg through PIL, resized like cv.resize) and becomes a pixel record.  Returns 'coef' | 'pixels'."""
    with open(path, 'rb') as f:
        data = f.read()
    rc = host_lib().dir_jpeg_decode_coefficients(data, len(data), row.ctypes.data, row.size)
    if rc == 0:
        hdr = row[:16].view(np.int32)
        if hdr[1] == size and hdr[2] == size:
            return 'coef'
    # -3 unsupported coding / -4 more coefficients than the ring's records hold (4:4:4 in a 4:2:0 ring) / another size: the host decodes this one
    if rc in (-1, -2):
        raise ValueError('%s: not a decodable JPEG (dir_jpeg_decode_coefficients returned %d)' % (path, rc))
    from .dataset import decode_bgr
    px = decode_bgr(path, size)
    need = HEADER_BYTES + px.size
    if row.size < need:
        raise ValueError('%s: a %d-byte record cannot hold the decoded %dx%d frame' % (path, row.size, size, size))
    row[:HEADER_BYTES] = 0
    hdr = row[:16].view(np.int32)
    hdr[0], hdr[1], hdr[2], hdr[3] = MAGIC_PIXELS, size, size, 3
    row[HEADER_BYTES:need] = px.reshape(-1)
    return 'pixels'


class RecordDecoder(object):
    """records on the GPU -> uint8 BGR frames [B,size,size,3] (dir_jpeg_decode_records), with its scratch planes and error word kept per instance"""

    def __init__(self, batch, stride, size=256, device='cuda'):
        """size: the frames' edge, or (height, width)"""
        self.batch, self.stride = batch, stride
        self.H, self.W = (size, size) if isinstance(size, int) else size
        L = _capi.lib()
        per = (int(L.dir_jpeg_planes_bytes(stride)) + 15) // 16 * 16
        self.scratch = torch.empty(batch * per, dtype=torch.uint8, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)

    def __call__(self, records, out, n=None):
        """records: uint8 cuda [B, stride]; out: uint8 cuda [B,size,size,3]; decodes the first n (default all) on the current stream"""
        _capi.require_cuda(records, out)
        assert records.dtype == torch.uint8 and records.is_contiguous() and records.shape[1] == self.stride and out.is_contiguous()
        n = records.shape[0] if n is None else n
        assert n <= self.batch and out.shape[0] >= n and tuple(out.shape[1:]) == (self.H, self.W, 3)
        with torch.cuda.device(records.device):
            _capi.check(_capi.lib().dir_jpeg_decode_records(_capi.ptr(records), self.stride, n, self.H, self.W, _capi.ptr(self.scratch), self.scratch.numel(),
                                                            _capi.ptr(out), _capi.ptr(self.err), _capi.stream_ptr()), 'dir_jpeg_decode_records')
        return out

    def check(self):
        """host read of the error word (a synchronisation: call it once per pass, not per batch)"""
        e = int(self.err.item())
        if e:
            raise _capi.DirHipError('dir_jpeg_decode_records: record %d of a batch did not describe a %dx%d image' % (e - 1, self.H, self.W))


def quality_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline) -> (luma, chroma) uint16 [64] in natural order (dir_jpeg_quality_tables)"""
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    if host_lib().dir_jpeg_quality_tables(int(quality), luma.ctypes.data, chroma.ctypes.data) != 0:
        raise ValueError('JPEG quality %r is not in 1..100' % (quality,))
    return luma, chroma


def record_to_bytes(row):
    """one coefficient record (a contiguous uint8 numpy array, at least the record's size) -> the bytes of its baseline JFIF file
    (dir_jpeg_encode_record: Huffman coding + file syntax on the host)"""
    lib = host_lib()
    row = np.ascontiguousarray(row, np.uint8)
    cap = int(lib.dir_jpeg_encode_bound(row.ctypes.data, row.size))
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_size_t(0)
    rc = lib.dir_jpeg_encode_record(row.ctypes.data, row.size, out.ctypes.data, cap, C.byref(n)) if cap else -2
    if rc != 0:
        raise ValueError('not an encodable coefficient record (dir_jpeg_encode_record returned %d)' % rc)
    return out[:n.value].tobytes()


def write_record(path, row):
    """one coefficient record -> a .jpg file"""
    data = record_to_bytes(row)
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


class RecordEncoder(object):
    """uint8 frames [B,H,W,3] on the GPU -> coefficient records on the GPU (dir_jpeg_encode_records), written into a caller's buffer
    [B, stride] uint8.  4:2:0, H and W multiples of 16 and at most 4096; the quantisation tables of `quality` are made once, on the host.
    A record becomes the file libjpeg writes for the frame at that quality through record_to_bytes / write_record."""

    def __init__(self, batch, size, quality=95, channel_order='bgr'):
        """size: the frames' edge, or (height, width); channel_order: 'bgr' (what cv.imwrite receives, the project's frames) or 'rgb'"""
        self.batch = batch
        self.H, self.W = (size, size) if isinstance(size, int) else size
        if channel_order not in ('bgr', 'rgb'):
            raise ValueError("channel_order must be 'bgr' or 'rgb'")
        self.order = 1 if channel_order == 'rgb' else 0
        self.quality = quality
        self.luma, self.chroma = quality_tables(quality)
        n = int(host_lib().dir_jpeg_record_bytes(self.W, self.H, 2, 2, 3))
        self.record_bytes = (n + 15) // 16 * 16

    def __call__(self, frames, records, n=None):
        """frames: uint8 cuda [B,H,W,3]; records: uint8 cuda [B, stride >= record_bytes]; encodes the first n (default all) on the current stream"""
        _capi.require_cuda(frames, records)
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and tuple(frames.shape[1:]) == (self.H, self.W, 3)
        assert records.dtype == torch.uint8 and records.is_contiguous() and records.dim() == 2
        n = frames.shape[0] if n is None else n
        assert n <= self.batch and frames.shape[0] >= n and records.shape[0] >= n
        with torch.cuda.device(frames.device):
            _capi.check(_capi.lib().dir_jpeg_encode_records(_capi.ptr(frames), n, self.H, self.W, self.order, self.luma.ctypes.data, self.chroma.ctypes.data,
                                                            _capi.ptr(records), records.shape[1], _capi.stream_ptr()), 'dir_jpeg_encode_records')
        return records


class RoundTrip(object):
    """frames -> records -> frames on the device (RecordEncoder + RecordDecoder, two entry points, buffers kept per instance): the pixels
    cv.imread / decode_bgr return from the file cv.imwrite writes for each frame at `quality`"""

    def __init__(self, batch, size=256, quality=95, channel_order='bgr', device='cuda'):
        self.enc = RecordEncoder(batch, size, quality, channel_order)
        self.dec = RecordDecoder(batch, self.enc.record_bytes, size, device)
        self.records = torch.empty(batch, self.enc.record_bytes, dtype=torch.uint8, device=device)

    def __call__(self, frames, out=None):
        """frames: uint8 cuda [B,H,W,3] in the encoder's channel order -> uint8 [B,H,W,3] in the same order (a new tensor unless `out` is given)"""
        n = frames.shape[0]
        out = torch.empty_like(frames) if out is None else out
        self.enc(frames, self.records, n)
        self.dec(self.records, out, n)                                   # (the decoder writes B, G, R)
        return out if self.enc.order == 0 else out.flip(-1)


_round_trips = {}


def jpeg_round_trip(frames, quality=95):
    """uint8 cuda BGR frames [B,H,W,3] -> the frames after cv.imwrite(quality) + cv.imread, computed on the device.  The RoundTrip instances
    (tables, record buffer, decoder scratch) are kept per (device, batch, size, quality)."""
    key = (frames.device, frames.shape[0], tuple(frames.shape[1:3]), int(quality))
    rt = _round_trips.get(key)
    if rt is None:
        rt = _round_trips[key] = RoundTrip(frames.shape[0], key[2], quality, 'bgr', frames.device)
    return rt(frames)
