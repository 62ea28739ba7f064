"""Hand crops from full frames on the GPU: csrc/crop.hip through dir_crop_matrices_from_boxes, dir_crop_matrices_from_meshes,
dir_crop_frames and dir_crop_frames_area.  The reference crops in one place only, dataset/dataset_utils.py:26-58 (cut_img, called by prepare_data.py:153-154 with the
ground-truth vertices and ratio 0.8); this is the same crop for frames of any size, from a box or from the previous frame's prediction,
and the way back from crop coordinates to frame pixels.  The rules are written out in include/dir_hip.h and restated in float64 numpy by
tests/helpers/crop_ref.py.

  crop_matrices_from_boxes    boxes [B,4] (x0, y0, x1, y1) -> (M float64 [B,6], valid int32 [B]), device tensors
  crop_matrices_from_meshes   one stage of DirEngine.forward + the matrices of its crops -> (M_next, valid): the tracking step
  FrameBatch                  HxWx3 uint8 BGR arrays of any sizes packed into one pinned buffer with their descriptors; one H2D copy
  crop_frames                 FrameBatch + M -> uint8 [B,size,size,3] = cv.warpAffine(frame, M, (size, size)), what DirEngine.forward takes;
                              antialias=True: where M shrinks the frame, Pillow's resize(BILINEAR, box) instead (no aliasing)
  to_frame_pixels             normalised crop uv [B,N,2] -> frame pixels
  frame_camera                (s, t) of uv = s xy + t -> (scale_px, trans_px) with frame pixel = scale_px xy + trans_px
  from_frame_pixels           frame pixels -> normalised crop uv: the float64 inverse of to_frame_pixels
  crop_camera                 (scale_px, trans_px) -> (s, tx, ty) of a crop: the float64 inverse of frame_camera
"""
import ctypes

import numpy as np
import torch

from .. import _capi

MIN_SIZE, MAX_SIZE, MAX_BATCH = 16, 1024, 4096          # DIR_CROP_MIN_SIZE, DIR_CROP_MAX_SIZE, DIR_CROP_MAX_BATCH
MAX_SIDE, MAX_STRIDE = 65536, 1 << 20                   # DIR_CROP_MAX_SIDE, DIR_CROP_MAX_STRIDE
STATUS_OK, STATUS_INVALID, STATUS_BAD_DESC, STATUS_BAD_MATRIX = 0, 1, 2, 3
FRAME_ALIGN = 16                                        # every image starts on a 16-byte boundary of the packed buffer
NV = 778
_DESC = np.dtype([('offset', '<i8'), ('height', '<i4'), ('width', '<i4'), ('row_stride', '<i8')])        # dir_frame_desc
assert _DESC.itemsize == ctypes.sizeof(_capi.FrameDesc) == 24


def _check_common(what, B, ratio, size):
    if not isinstance(size, int) or not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError('%s: size must be an int in %d..%d, got %r' % (what, MIN_SIZE, MAX_SIZE, size))
    if not 0 < float(ratio) <= 16:
        raise ValueError('%s: ratio must be in (0, 16], got %r' % (what, ratio))
    if not 1 <= B <= MAX_BATCH:
        raise ValueError('%s: the batch must hold 1..%d images, got %d' % (what, MAX_BATCH, B))


def crop_matrices_from_boxes(boxes, ratio=0.8, size=256):
    """dir_crop_matrices_from_boxes: boxes cuda [B,4] = (x0, y0, x1, y1), the tight box around both hands in frame pixel positions ->
    (M float64 [B,6], valid int32 [B]).  The hands fill `ratio` of the crop's side, as cut_img(..., radio=ratio) makes them.  An invalid
    row (not finite, zero area, a scale outside 2^-6 .. 2^6, a corner beyond 2^20 px) has a zero matrix."""
    _capi.require_cuda(boxes)
    boxes = _capi.f32c(boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError('crop_matrices_from_boxes: need boxes [B,4], got %s' % (tuple(boxes.shape),))
    B, dev = boxes.shape[0], boxes.device
    _check_common('crop_matrices_from_boxes', B, ratio, size)
    M, valid = torch.empty(B, 6, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_crop_matrices_from_boxes(P(boxes), B, float(ratio), size, P(M), P(valid), _capi.stream_ptr()),
                    'dir_crop_matrices_from_boxes')
    return M, valid


def _check_matrix(what, M, B, dev):
    if not isinstance(M, torch.Tensor) or M.dtype != torch.float64 or tuple(M.shape) != (B, 6) or not M.is_contiguous() or M.device != dev:
        raise ValueError('%s: the matrices must be a contiguous float64 [%d,6] tensor on %s' % (what, B, dev))


def crop_matrices_from_meshes(stage, M_prev, ratio=0.8, size=256):
    """dir_crop_matrices_from_meshes, the tracking step: `stage` is one stage of DirEngine.forward's output for crops made with M_prev
    (float64 [B,6]); -> (M_next float64 [B,6], valid int32 [B]): the crop that holds the projected meshes of both hands at `ratio` of
    its side.  Where no such crop exists (a non-finite prediction, a collapsed or exploded one) M_next = M_prev and valid = 0."""
    t = [_capi.f32c(stage[k]) for k in ('pd_mesh_xyz_left', 'pd_mesh_xyz_right', 'pd_proj_left', 'pd_proj_right')]
    _capi.require_cuda(M_prev, *t)
    B, dev = t[0].shape[0], t[0].device
    if any(tuple(m.shape) != (B, NV, 3) for m in t[:2]) or any(tuple(p.shape) != (B, 3) for p in t[2:]) or any(x.device != dev for x in t):
        raise ValueError('crop_matrices_from_meshes: need pd_mesh_xyz_* [B,778,3] and pd_proj_* [B,3] on one device, got %s' % [tuple(x.shape) for x in t])
    _check_common('crop_matrices_from_meshes', B, ratio, size)
    _check_matrix('crop_matrices_from_meshes', M_prev, B, dev)
    M, valid = torch.empty(B, 6, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_crop_matrices_from_meshes(P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(M_prev), B, float(ratio), size, P(M), P(valid),
                                                              _capi.stream_ptr()), 'dir_crop_matrices_from_meshes')
    return M, valid


def check_descs(descs, nbytes):
    """the kernel's own descriptor rule, on the host: ValueError for the first (offset, height, width, row_stride) that breaks it"""
    for i, (off, h, w, stride) in enumerate(descs):
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and 3 * w <= stride <= MAX_STRIDE and 0 <= off <= nbytes and
                (h - 1) * stride + 3 * w <= nbytes - off):
            raise ValueError('FrameBatch: image %d (offset %d, %d x %d, row stride %d) does not lie inside a buffer of %d bytes with '
                             'sides in 1..%d and 3 * width <= row stride <= %d' % (i, off, h, w, stride, nbytes, MAX_SIDE, MAX_STRIDE))


class FrameBatch(object):
    """A ragged batch of uint8 BGR frames for crop_frames: `buffer` (numpy uint8) holds the images, each on a FRAME_ALIGN boundary with
    rows of 3 * width bytes, followed by the descriptor table, so that cuda() is ONE host-to-device copy (from pinned memory).
    descs: [(offset, height, width, row_stride)]; sizes: [(height, width)].  from_buffer() takes a packed buffer and descriptors as they
    are (rows may be padded).  Both check every descriptor against the kernel's own rule (check_descs) and raise ValueError."""

    def __init__(self, frames):
        frames = list(frames)
        if not 1 <= len(frames) <= MAX_BATCH:
            raise ValueError('FrameBatch: need 1..%d frames, got %d' % (MAX_BATCH, len(frames)))
        descs, off = [], 0
        for i, f in enumerate(frames):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or 0 in f.shape:
                raise ValueError('FrameBatch: frame %d must be a non-empty uint8 array [H,W,3], got %s' % (
                    i, (f.dtype, f.shape) if isinstance(f, np.ndarray) else type(f)))
            descs.append((off, f.shape[0], f.shape[1], 3 * f.shape[1]))
            off = -(-(off + f.size) // FRAME_ALIGN) * FRAME_ALIGN
        check_descs(descs, off)                                              # a frame wider than MAX_SIDE or MAX_STRIDE / 3 is refused here
        self._init(None, descs, off)
        for f, (o, h, w, stride) in zip(frames, descs):
            self.buffer[o:o + h * stride].reshape(h, w, 3)[...] = f

    @classmethod
    def from_buffer(cls, buffer, descs, validate=True):
        """a packed uint8 buffer (numpy, 1-D) and its descriptors.  validate=False skips the host check: the kernel applies the same rule
        and answers a descriptor that breaks it with a zero crop and DIR_CROP_BAD_DESC"""
        buffer = np.ascontiguousarray(buffer)
        if buffer.dtype != np.uint8 or buffer.ndim != 1 or buffer.size == 0:
            raise ValueError('FrameBatch.from_buffer: need a non-empty 1-D uint8 buffer')
        descs = [tuple(int(v) for v in d) for d in descs]
        if not 1 <= len(descs) <= MAX_BATCH or any(len(d) != 4 for d in descs):
            raise ValueError('FrameBatch.from_buffer: need 1..%d descriptors (offset, height, width, row_stride)' % MAX_BATCH)
        if validate:
            check_descs(descs, buffer.size)
        self = cls.__new__(cls)
        self._init(buffer, descs, buffer.size)
        return self

    def _init(self, data, descs, nbytes):
        self.descs, self.nbytes = descs, int(nbytes)
        self.sizes = [(d[1], d[2]) for d in descs]
        self._desc_off = -(-self.nbytes // 8) * 8                            # the table is read as 8-byte fields
        total = self._desc_off + len(descs) * _DESC.itemsize
        self._host = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        self.buffer = self._host.numpy()
        self.buffer[self.nbytes:self._desc_off] = 0
        if data is not None:
            self.buffer[:self.nbytes] = data
        self.buffer[self._desc_off:] = np.array(descs, dtype=_DESC).view(np.uint8)
        self._dev = None

    def __len__(self):
        return len(self.descs)

    def cuda(self, device='cuda'):
        """-> the device copy of the whole buffer (uint8), made once"""
        device = torch.device(device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._dev is None or self._dev.device != device:
            self._dev = self._host.to(device, non_blocking=True)
        return self._dev


def crop_frames(batch, M, valid=None, size=256, return_status=False, antialias=False, return_area=False):
    """dir_crop_frames: batch a FrameBatch, M float64 cuda [B,6] (OpenCV's convention: crop position = M * frame position), valid int32
    cuda [B] or None -> uint8 cuda [B,size,size,3], byte for byte cv.warpAffine(frame, M, (size, size)) with INTER_LINEAR and a zero
    border.  An image whose `valid` is 0, whose descriptor reaches outside the buffer or whose matrix sends a crop pixel beyond 2^20 px
    gives an all-zero crop; with return_status -> (crops, status int32 [B]: 0 or STATUS_INVALID / STATUS_BAD_DESC / STATUS_BAD_MATRIX).

    antialias=True (dir_crop_frames_area): an image whose matrix shrinks the frame (no rotation, shear or mirror, both scales positive,
    the smaller one below 1) is resampled with a triangle filter as wide as the shrink -- byte for byte Pillow's
    Image.resize((size, size), BILINEAR, box) on the box the matrix cuts out, with the same zero border -- and every other image is the
    crop above, byte for byte.  A shrinking scale below 2^-6 is STATUS_BAD_MATRIX.  With return_area the tuple ends with area int32 [B]:
    1 where the anti-aliased rule was used.  -> crops, or (crops[, status][, area])."""
    if not isinstance(batch, FrameBatch):
        raise ValueError('crop_frames: batch must be a FrameBatch')
    if return_area and not antialias:
        raise ValueError('crop_frames: return_area needs antialias=True')
    _capi.require_cuda(M, valid)
    B, dev = len(batch), M.device
    _check_common('crop_frames', B, 1.0, size)
    _check_matrix('crop_frames', M, B, dev)
    if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (B,) or not valid.is_contiguous() or valid.device != dev):
        raise ValueError('crop_frames: valid must be a contiguous int32 [%d] tensor on %s' % (B, dev))
    buf = batch.cuda(dev)
    out = torch.empty(B, size, size, 3, dtype=torch.uint8, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    P = _capi.ptr
    descs = ctypes.c_void_p(buf.data_ptr() + batch._desc_off)
    area = torch.empty(B, dtype=torch.int32, device=dev) if return_area else None
    with torch.cuda.device(dev):
        if antialias:
            _capi.check(_capi.lib().dir_crop_frames_area(P(buf), batch.nbytes, descs, P(M), P(valid), B, size, P(out), P(status), P(area),
                                                         _capi.stream_ptr()), 'dir_crop_frames_area')
        else:
            _capi.check(_capi.lib().dir_crop_frames(P(buf), batch.nbytes, descs, P(M), P(valid), B, size, P(out), P(status), _capi.stream_ptr()),
                        'dir_crop_frames')
    res = (out,) + ((status,) if return_status else ()) + ((area,) if return_area else ())
    return res if len(res) > 1 else out


def to_frame_pixels(uv, M, size=256):
    """normalised crop coordinates uv [B,N,2] (-1..1 over the crop, as pd_joint_uv_*) -> frame pixel positions float32 [B,N,2]:
    ((uv + 1) size / 2 - M[:, (2, 5)]) / M[:, 0] in float64, rounded once.  A zero matrix (an invalid crop) gives non-finite values."""
    M = M.reshape(-1, 6)
    c = (uv.double() + 1.0) * float(size) / 2.0
    return ((c - M[:, None, (2, 5)]) / M[:, None, 0:1]).float()


def frame_camera(proj, M, size=256):
    """proj [B,3] = (s, tx, ty) of uv = s xy + t (pd_proj_*) -> (scale_px float32 [B], trans_px float32 [B,2]) with
    frame pixel = scale_px xy + trans_px, in float64 and rounded once"""
    M = M.reshape(-1, 6)
    p = proj.double()
    scale = p[:, 0] * float(size) / 2.0 / M[:, 0]
    trans = ((p[:, 1:3] + 1.0) * float(size) / 2.0 - M[:, (2, 5)]) / M[:, 0:1]
    return scale.float(), trans.float()


def from_frame_pixels(px, M, size=256):
    """frame pixel positions [B,N,2] -> normalised crop coordinates of the crop M, float64 [B,N,2]: (px M[:, 0] + M[:, (2, 5)]) 2 / size - 1,
    the inverse of to_frame_pixels in float64, NOT rounded to float32 (the caller rounds once)"""
    M = M.reshape(-1, 6)
    return (px.double() * M[:, None, 0:1] + M[:, None, (2, 5)]) * 2.0 / float(size) - 1.0


def crop_camera(scale_px, trans_px, M, size=256):
    """(scale_px [B], trans_px [B,2]) with frame pixel = scale_px xy + trans_px -> proj float64 [B,3] = (s, tx, ty) with uv = s xy + t in the
    crop M: the inverse of frame_camera in float64, NOT rounded to float32 (the caller rounds once)"""
    M = M.reshape(-1, 6)
    s = scale_px.double() * M[:, 0] * 2.0 / float(size)
    t = (trans_px.double() * M[:, 0:1] + M[:, (2, 5)]) * 2.0 / float(size) - 1.0
    return torch.cat((s[:, None], t), 1)
