"""CPU: the JPEG ENCODE pieces that need no GPU.

  * tests/helpers/jpeg_enc_ref.py (numpy restatement, int64, of libjpeg's default compression: quality tables, colour conversion, h2v2
    downsampling, islow forward DCT, quantisation, Huffman coding, file syntax) is PINNED to the bytes the real libjpeg-turbo wrote for the
    committed frames (tests/golden/g26_jpeg_enc.npz, written by tools/gen_jpeg_enc_golden.py through Pillow): byte for byte; and, where Pillow
    is importable, to Pillow itself on freshly written files.  Its records equal what the host decoder reads from those files, header included.
  * every intermediate of its DCT lies inside int32 on saturated frames: the arithmetic csrc/jpeg_enc.hip uses.
  * lib/libdir_jpeg.so's encode half (csrc/jpeg_enc_huff.c, include/dir_jpeg_enc.h): quality tables, record -> file equal to the golden bytes,
    decode -> encode -> decode of every baseline file of g22_jpeg.npz, space and range errors, exported symbols, and a few thousand corrupt
    records in a child process."""
import ctypes as C
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import jpeg as J

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import jpeg_enc_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'g26_jpeg_enc.npz')
GOLD_DEC = os.path.join(ROOT, 'tests', 'golden', 'g22_jpeg.npz')
OK, E_ARG, E_FORMAT, E_UNSUPPORTED, E_SPACE = 0, -1, -2, -3, -4


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    names = sorted(k[:-6] for k in g.files if k.endswith('.frame'))
    assert len(names) >= 15
    return {n: dict(frame=g[n + '.frame'], q=int(g[n + '.q']), jpg=g[n + '.jpg'].tobytes(), pix=g[n + '.pix']) for n in names}


@pytest.fixture(scope='module')
def records(gold):
    """the restatement's record of every golden frame, computed once"""
    return {n: R.encode_record(c['frame'], c['q']) for n, c in gold.items()}


@pytest.fixture(scope='module')
def lib():
    from dir_amd import build
    from dir_amd.apps import jpeg as AJ
    build.build_jpeg_host(verbose=False)
    return AJ.host_lib()


def decode_record(lib, data, nbytes):
    rec = np.zeros(nbytes, np.uint8)
    assert lib.dir_jpeg_decode_coefficients(data, len(data), rec.ctypes.data, rec.size) == OK
    return rec


def encode(lib, rec, cap=None):
    cap = int(lib.dir_jpeg_encode_bound(rec.ctypes.data, rec.size)) if cap is None else cap
    out = np.full(cap + 64, 0xA5, np.uint8)
    n = C.c_size_t(0)
    rc = lib.dir_jpeg_encode_record(rec.ctypes.data, rec.size, out.ctypes.data, cap, C.byref(n))
    assert (out[cap:] == 0xA5).all(), 'wrote past cap'
    return rc, out[:n.value].tobytes()


def test_golden_covers_the_cases(gold):
    shapes = {(c['frame'].shape[:2], c['q']) for c in gold.values()}
    for want in (((16, 16), 75), ((32, 48), 95), ((48, 32), 50), ((256, 256), 95)):
        assert want in shapes
    assert {c['q'] for n, c in gold.items() if n.startswith('checker')} == {1, 100}
    for c in gold.values():
        assert c['frame'].dtype == np.uint8 and c['frame'].shape[0] % 16 == 0 and c['frame'].shape[1] % 16 == 0


def test_restatement_files_equal_libjpeg_turbo(gold):
    for n, c in gold.items():
        assert R.encode_file(c['frame'], c['q']) == c['jpg'], n
    # the channel-order argument: the same picture handed over as RGB
    c = gold['noise_32x48_q95']
    assert R.encode_file(np.ascontiguousarray(c['frame'][..., ::-1]), c['q'], 'rgb') == c['jpg']


def test_restatement_files_equal_pillow_on_fresh_files():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(3)
    for h, w, q in ((16, 16, 75), (32, 32, 95), (48, 32, 100), (64, 64, 30), (16, 48, 1), (32, 16, 49), (16, 32, 51)):
        a = np.clip(rng.normal(128, 90, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format='JPEG', quality=q, subsampling=2)
        assert R.encode_file(a, q, 'rgb') == buf.getvalue(), (h, w, q)


def test_restatement_records_equal_the_host_decode_of_the_golden_files(gold, records, lib):
    for n, c in gold.items():
        rec = records[n]
        H, W = c['frame'].shape[:2]
        assert rec.size == 512 + H * W * 3 == lib.dir_jpeg_record_bytes(W, H, 2, 2, 3), n
        want = decode_record(lib, c['jpg'], rec.size)
        assert np.array_equal(rec[:512], want[:512]), n                      # all 512 header bytes
        assert np.array_equal(rec[512:], want[512:]), n                      # every coefficient
        info, coef = J.decode_coefficients(c['jpg'])
        assert np.array_equal(rec[512:].view(np.int16), np.concatenate([k.reshape(-1) for k in coef])), n


def test_dct_intermediates_of_saturated_frames_fit_int32(gold):
    """libjpeg's analysis says 32 bits suffice for 8-bit samples; csrc/jpeg_enc.hip relies on it"""
    worst = 0
    frames = [c['frame'] for n, c in gold.items() if n.startswith(('checker', 'const', 'rects'))]
    yy, xx = np.mgrid[0:16, 0:16]
    for k in range(8):                                                    # the basis functions' sign patterns at full swing, per channel
        for l in range(8):
            s = (np.cos((2 * yy + 1) * k * np.pi / 16) * np.cos((2 * xx + 1) * l * np.pi / 16) >= 0)
            frames.append(np.stack([s, ~s, s], -1).astype(np.uint8) * 255)
            frames.append(np.stack([s, s, s], -1).astype(np.uint8) * 255)
    for f in frames:
        track = [0]
        R.coefficients(f, 100, track=track)
        worst = max(worst, track[0])
    assert 0 < worst < 2 ** 31 - 1, worst
    assert worst < 2 ** 29, worst                                         # and with room to spare


def test_quality_tables(gold, lib):
    Image = None
    try:
        from PIL import Image
    except ImportError:
        pass
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    for q in (1, 25, 50, 75, 95, 100):
        assert lib.dir_jpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data) == OK
        ql, qc = R.quality_tables(q)
        assert np.array_equal(luma, ql) and np.array_equal(chroma, qc), q
        if Image is not None:
            buf = io.BytesIO()
            Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format='JPEG', quality=q, subsampling=2)
            qt = J.parse(buf.getvalue())['qt']
            assert np.array_equal(luma, qt[0]) and np.array_equal(chroma, qt[1]), q
    for n, c in gold.items():                                             # and the tables inside the committed files
        qt = J.parse(c['jpg'])['qt']
        assert lib.dir_jpeg_quality_tables(c['q'], luma.ctypes.data, chroma.ctypes.data) == OK
        assert np.array_equal(luma, qt[0]) and np.array_equal(chroma, qt[1]), n
    for q in (0, 101, -5):
        assert lib.dir_jpeg_quality_tables(q, luma.ctypes.data, chroma.ctypes.data) == E_ARG


def test_host_encoder_writes_the_golden_bytes(gold, records, lib):
    from dir_amd.apps import jpeg as AJ
    for n, c in gold.items():
        rc, data = encode(lib, records[n])
        assert rc == OK and data == c['jpg'], n
        assert AJ.record_to_bytes(records[n]) == c['jpg'], n
        padded = np.concatenate([records[n], np.full(48, 0xA5, np.uint8)])   # a slot larger than its record
        assert AJ.record_to_bytes(padded) == c['jpg'], n


def test_decode_encode_decode_of_every_baseline_file(lib):
    """generic over what the header describes: 4:4:4, 4:2:2, 4:2:0, grayscale, odd sizes, files with restart intervals"""
    g = np.load(GOLD_DEC)
    names = sorted(k[:-4] for k in g.files if k.endswith('.rgb'))
    assert len(names) >= 12
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for n in names:
        data = g[n + '.jpg'].tobytes()
        H, W = g[n + '.rgb'].shape[:2]
        nbytes = 512 + 3 * ((H + 15) // 16 * 16) * ((W + 15) // 16 * 16) * 2
        rec = decode_record(lib, data, nbytes)
        rc, again = encode(lib, rec)
        assert rc == OK, n
        rec2 = decode_record(lib, again, nbytes)
        assert np.array_equal(rec, rec2), n
        assert np.array_equal(J.decode(again), g[n + '.rgb']), n
        hdr = rec[:96].view(np.int32)
        nc = int(hdr[3])
        coef = [rec[512:].view(np.int16)[hdr[20 + c]:hdr[20 + c] + hdr[14 + c] * hdr[17 + c] * 64].reshape(hdr[17 + c], hdr[14 + c], 64) for c in range(nc)]
        quants = [rec[96 + 128 * c:224 + 128 * c].view(np.uint16) for c in range(nc)]
        assert R.file_from(int(hdr[1]), int(hdr[2]), [int(x) for x in hdr[8:8 + nc]], [int(x) for x in hdr[11:11 + nc]], quants, coef) == again, n
        if Image is not None:
            with Image.open(io.BytesIO(again)) as im:
                assert np.array_equal(np.asarray(im.convert('RGB')), g[n + '.rgb']), n


def test_space_and_range_errors(gold, records, lib):
    rec = records['noise_16x16_q75']
    full = len(gold['noise_16x16_q75']['jpg'])
    assert lib.dir_jpeg_encode_bound(rec.ctypes.data, rec.size) >= full
    for cap in (full - 1, full // 2, 700, 100, 1, 0):                      # one byte short, inside the scan, inside the tables, ...
        rc, data = encode(lib, rec, cap)                                  # (encode() checks the guard bytes behind cap)
        assert rc == E_SPACE and data == b'', cap
    assert encode(lib, rec, full)[0] == OK
    for pos, val, want in ((1, 1024, E_FORMAT), (1, -1024, E_FORMAT), (1, 1023, OK), (63, -1023, OK), (0, 2048, E_FORMAT), (0, -2048, E_FORMAT),
                           (0, 2047, OK), (64, 4000, E_FORMAT), (64 * 4, -3000, E_FORMAT)):
        bad = rec.copy()
        co = bad[512:].view(np.int16)
        co[:] = 0
        co[pos] = val
        rc, data = encode(lib, bad)
        assert rc == want, (pos, val, rc)
        if want == OK:
            assert np.array_equal(decode_record(lib, data, bad.size), bad)
    n = C.c_size_t(0)
    out = np.zeros(4096, np.uint8)
    assert lib.dir_jpeg_encode_record(None, rec.size, out.ctypes.data, out.size, C.byref(n)) == E_ARG
    assert lib.dir_jpeg_encode_record(rec.ctypes.data, 100, out.ctypes.data, out.size, C.byref(n)) == E_ARG
    assert lib.dir_jpeg_encode_record(rec.ctypes.data, rec.size - 2, out.ctypes.data, out.size, C.byref(n)) == E_FORMAT     # shorter than total_coef
    big = rec.copy()
    big[96:98].view(np.uint16)[0] = 300
    assert encode(lib, big, 4096)[0] == E_UNSUPPORTED
    big[96:98].view(np.uint16)[0] = 0
    assert encode(lib, big, 4096)[0] == E_FORMAT


def test_encoder_header_is_exported():
    from dir_amd import build
    build.build_jpeg_host(verbose=False)
    lib = C.CDLL(build.JPEG_LIB)
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dir_jpeg_enc.h')).read(), flags=re.S)
    syms = sorted(set(re.findall(r'\b(dir_jpeg_[a-z0-9_]+)\s*\(', src)))
    assert syms == ['dir_jpeg_enc_abi_version', 'dir_jpeg_encode_bound', 'dir_jpeg_encode_record', 'dir_jpeg_quality_tables']
    for s in syms:
        assert hasattr(lib, s)
    assert lib.dir_jpeg_enc_abi_version() == int(re.search(r'#define\s+DIR_JPEG_ENC_ABI_VERSION\s+(\d+)', src).group(1))
    # the decode header keeps its own version
    dec = open(os.path.join(ROOT, 'include', 'dir_jpeg.h')).read()
    assert lib.dir_jpeg_abi_version() == int(re.search(r'#define\s+DIR_JPEG_ABI_VERSION\s+(\d+)', dec).group(1)) == 1


def test_host_encoder_survives_corrupt_records(lib):
    """the encode workers read records from a buffer another process filled: corrupt headers, lengths and coefficients must come back as an
    error code (or encode to something) -- never crash, never write past cap.  4 000 mutations in a child process (a segfault there is a
    failure here), with guard bytes behind every output buffer."""
    code = r'''
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, 'tests', 'helpers'))
from dir_amd.apps import jpeg as AJ
lib = AJ.host_lib()
g = np.load(%r)
recs = []
for k in g.files:
    if k.endswith('.jpg') and not k.startswith('progressive'):
        d = g[k].tobytes()
        r = np.zeros(1 << 18, np.uint8)
        if lib.dir_jpeg_decode_coefficients(d, len(d), r.ctypes.data, r.size) == 0:
            recs.append(r[:512 + 2 * int(r[92:96].view(np.int32)[0])].copy())
assert len(recs) >= 10
rng = np.random.RandomState(13)
out = np.empty((1 << 20) + 64, np.uint8)
codes = {}
for it in range(4000):
    r = recs[it %% len(recs)].copy()
    kind = it %% 4
    if kind == 0:                                   # one header word replaced (geometry, sampling, offsets, tables)
        r[:512].view(np.int32)[rng.randint(0, 128)] = [0, -1, 1, 2, 3, 65536, 2 ** 31 - 1, -2 ** 31, rng.randint(-70000, 70000)][rng.randint(0, 9)]
    elif kind == 1:                                 # a few header bytes flipped
        for _ in range(rng.randint(1, 6)):
            r[rng.randint(0, 512)] = rng.randint(0, 256)
    elif kind == 2:                                 # the record cut short / its length misreported
        r = r[:rng.randint(0, r.size)].copy()
    else:                                           # coefficients out of range
        co = r[512:].view(np.int16)
        for _ in range(rng.randint(1, 8)):
            co[rng.randint(0, co.size)] = rng.randint(-32768, 32768)
    nb = r.size if kind != 2 or rng.randint(0, 2) else r.size + rng.randint(1, 4096)      # (kind 2, sometimes: a length beyond the buffer's end is
    buf = np.zeros(max(nb, 1) + 8192, np.uint8)                                           #  still inside this allocation: no read fault, only the code)
    buf[:r.size] = r
    cap = [1 << 20, 4096, 700, 64, 0][rng.randint(0, 5)]
    out[cap:cap + 64] = 0xA5
    n = C.c_size_t(0)
    rc = lib.dir_jpeg_encode_record(buf.ctypes.data, nb, out.ctypes.data, cap, C.byref(n))
    assert (out[cap:cap + 64] == 0xA5).all(), ('wrote past cap', it, cap, rc)
    assert rc in (0, -1, -2, -3, -4) and n.value <= cap, (rc, n.value, cap)
    bound = lib.dir_jpeg_encode_bound(buf.ctypes.data, nb)
    assert rc != 0 or cap < bound or n.value <= bound
    codes[rc] = codes.get(rc, 0) + 1
print('codes', sorted(codes.items()))
''' % (ROOT, ROOT, GOLD_DEC)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert 'codes' in r.stdout
    codes = dict(eval(r.stdout.split('codes', 1)[1]))
    assert codes.get(0, 0) > 0 and codes.get(-2, 0) > 0 and codes.get(-4, 0) > 0, codes
