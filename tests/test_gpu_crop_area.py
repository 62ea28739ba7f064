"""GPU: anti-aliased hand crops (dir_crop_frames_area through dir_amd.utils.crop.crop_frames(antialias=True)).

  pixels       the kernel == tests/helpers/crop_area_ref.py::crop_area byte for byte on one ragged batch (five frames, two of them views
               with padded rows, one of those with rows that start on every byte phase) that mixes shrinking matrices at s = 1/2, 0.3,
               1/7.3, 3/64 and exactly 1/64, anisotropic ones with one axis >= 1, boxes partly and wholly outside the frame, and
               matrices that keep the plain rule (s = 1, 1.7, a rotation); crops of 16, and of 17 with B = 3, where tiles, lanes and dword
               stores straddle rows and images
  default      antialias=False, and the non-shrinking images with it on, are dir_crop_frames' own bytes
  invariance   an image gives the same bytes alone, first and last in a batch
  statuses     valid = 0, a descriptor past the buffer, a non-finite matrix, a scale below 2^-6: a black crop and the status
  C ABI        a null pointer, B or size out of range, a misaligned `out`: a negative code, nothing launched

The integer sums are exact and every coefficient is made of correctly rounded IEEE double operations in one order, so the comparison has
no tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_area_ref as A  # noqa: E402

from dir_amd.utils import crop as CR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(40, 53), (97, 64), (128, 96), (300, 200), (61, 301)]          # (H, W); 2 and 4 are views of wider parents


def make_frames(seed=4600):
    """-> (frames, buf, descs): five seeded frames in one packed buffer.  Frame 2 starts 9 bytes into a parent 10 px wider; frame 4 lies in
    a parent 2 px wider, so its rows (909 bytes apart) start on every byte phase of a dword"""
    rng = np.random.default_rng(seed)
    frames, chunks, descs, off = [], [], [], 0
    for k, (h, w) in enumerate(SHAPES):
        extra, lead = {2: (10, 3), 4: (2, 1)}.get(k, (0, 0))
        parent = rng.integers(0, 256, (h, w + extra, 3)).astype(np.uint8)
        frames.append(parent[:, lead:lead + w])
        descs.append((off + 3 * lead, h, w, 3 * (w + extra)))
        n = -(-parent.size // 16) * 16
        chunks.append(np.concatenate([parent.reshape(-1), np.zeros(n - parent.size, np.uint8)]))
        off += n
    return frames, np.concatenate(chunks), descs


def centred(frame, size, sx, sy=None, dx=0.0, dy=0.0):
    """the axis-aligned matrix of scales (sx, sy) whose crop is centred on the frame's centre moved by (dx, dy) frame pixels"""
    sy = sx if sy is None else sy
    h, w = frame.shape[:2]
    return np.array([[sx, 0.0, size / 2 - sx * (w / 2 + dx)], [0.0, sy, size / 2 - sy * (h / 2 + dy)]])


def cases(frames, size):
    """-> [(frame index, matrix)]"""
    c, s = np.cos(0.4), np.sin(0.4)
    f = frames
    return [
        (0, centred(f[0], size, 0.5)),                                   # inside
        (3, centred(f[3], size, 0.3, dx=1.37, dy=-2.21)),
        (4, centred(f[4], size, 1 / 7.3, dx=20.5)),                      # wider than the frame is high: rows outside above and below
        (3, centred(f[3], size, 3 / 64)),                                # the frame is a few crop pixels in the middle
        (3, centred(f[3], size, 2.0 ** -6, dx=-17.0, dy=9.0)),           # exactly DIR_CROP_MIN_SCALE: 129 taps
        (2, centred(f[2], size, 0.5, 1.5)),                              # anisotropic: y is not shrunk (2 or 3 taps)
        (1, centred(f[1], size, 2.0, 0.25)),
        (2, centred(f[2], size, 0.4, dx=-60.0, dy=-70.0)),               # the box hangs over the top left corner
        (4, centred(f[4], size, 0.6, dx=150.0, dy=28.0)),                # ... and over the bottom right one, odd row phases
        (1, np.array([[0.5, 0.0, 5000.0], [0.0, 0.5, 5000.0]])),         # wholly outside
        (0, np.array([[1.0, 0.0, -3.0], [0.0, 1.0, -2.0]])),             # the plain rule from here on
        (1, centred(f[1], size, 1.7)),
        (2, np.array([[0.5 * c, 0.5 * s, 3.0], [-0.5 * s, 0.5 * c, 20.0]])),
        (4, centred(f[4], size, 0.25)),                                  # and a shrinking one last in the batch
    ]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def scene():
    frames, buf, descs = make_frames()
    return {'frames': frames, 'buf': buf, 'descs': descs}


_REF = {}


def reference(scene, size):
    """crop_area of every case, computed once per size and shared: (cases, crops uint8 [n,size,size,3], area flags)"""
    if size not in _REF:
        cs = cases(scene['frames'], size)
        _REF[size] = (cs, np.stack([A.crop_area(scene['frames'][k], M, size) for k, M in cs]), [int(A.is_shrinking(M)) for _, M in cs])
    return _REF[size]


def batch_of(scene, idx):
    return CR.FrameBatch.from_buffer(scene['buf'], [scene['descs'][k] for k in idx])


def run(scene, cs, size, antialias=True):
    out = CR.crop_frames(batch_of(scene, [k for k, _ in cs]), dev(np.stack([M for _, M in cs]).reshape(-1, 6)), size=size, return_status=True,
                         antialias=antialias, return_area=antialias)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def differing(got, want):
    bad = (got != want).any(-1)
    return int(bad.sum()), np.argwhere(bad)[:4].tolist()


def test_kernel_equals_crop_area_byte_for_byte(scene):
    cs, want, flags = reference(scene, 16)
    got, status, area = run(scene, cs, 16)
    assert got.shape == want.shape and got.dtype == np.uint8 and not status.any()
    assert area.tolist() == flags == [1] * 9 + [1, 0, 0, 0, 1]
    for j in range(len(cs)):
        assert np.array_equal(got[j], want[j]), (j, cs[j][1].tolist()) + differing(got[j], want[j])
    assert not want[9].any() and all(want[j].any() for j in range(len(cs)) if j != 9)
    assert not want[7][:4, :4].any() and want[7][-4:, -4:].all()        # the corner outside is border, the corner inside is image


@pytest.mark.parametrize('first', [0, 3, 6, 9, 11])
def test_crops_of_17_in_batches_of_three(scene, first):
    """289 pixels per crop: the second column tile is one pixel wide, the second row band one row high, the plain kernel's lanes of
    four pixels straddle images that the other kernel owns"""
    cs, want, flags = reference(scene, 17)
    got, status, area = run(scene, cs[first:first + 3], 17)
    assert got.shape == (3, 17, 17, 3) and not status.any() and area.tolist() == flags[first:first + 3]
    for j in range(3):
        assert np.array_equal(got[j], want[first + j]), (first + j,) + differing(got[j], want[first + j])


def test_default_and_plain_images_are_dir_crop_frames_bytes(scene):
    cs, _, flags = reference(scene, 16)
    plain, st0 = run(scene, cs, 16, antialias=False)
    base = CR.crop_frames(batch_of(scene, [k for k, _ in cs]), dev(np.stack([M for _, M in cs]).reshape(-1, 6)), size=16).cpu().numpy()
    assert np.array_equal(plain, base) and not st0.any()                # the default arguments and antialias=False: one path
    got, _, area = run(scene, cs, 16)
    for j, fl in enumerate(flags):
        assert np.array_equal(got[j], plain[j]) == (fl == 0 or not plain[j].any()), j        # shrinking images differ (the empty one aside)
    assert flags.count(0) == 3
    with pytest.raises(ValueError):
        CR.crop_frames(batch_of(scene, [0]), dev(np.eye(2, 3).reshape(1, 6)), size=16, return_area=True)      # no flags without antialias


def test_batch_invariance(scene):
    cs, want, _ = reference(scene, 16)
    for j in (1, 4, 8):                                                 # s = 0.3, 1/64, odd row phases
        others = [cs[0], cs[12], cs[5]]
        alone = run(scene, [cs[j]], 16)[0][0]
        first = run(scene, [cs[j]] + others, 16)[0][0]
        last = run(scene, others + [cs[j]], 16)[0][-1]
        assert np.array_equal(alone, want[j]) and np.array_equal(first, alone) and np.array_equal(last, alone), j


def test_refused_images_are_black(scene):
    """the bad descriptor's frame is the LAST of the buffer and claims more rows than it has, so an unchecked read would leave the buffer;
    the assertion is the status and the zero crop"""
    cs, want, _ = reference(scene, 16)
    use = [cs[1], cs[0], cs[8], cs[2], cs[5], cs[13]]                   # frames 3, 0, 4, 4, 2, 4
    M = np.stack([m for _, m in use]).reshape(-1, 6).copy()
    descs = [scene['descs'][k] for k, _ in use]
    off, h, w, stride = descs[2]
    descs[2] = (off, h + 40, w, stride)                                 # reaches 36 000 bytes past the end
    M[3] = [np.nan, 0, 0, 0, 0.5, 0]
    M[4] = [2.0 ** -6 * 0.99, 0, 8.0, 0, 1.5, 0]                        # a shrinking matrix below DIR_CROP_MIN_SCALE
    valid = dev(np.int32([1, 0, 1, 1, 1, 1]))
    with pytest.raises(ValueError):
        CR.FrameBatch.from_buffer(scene['buf'], descs)
    batch = CR.FrameBatch.from_buffer(scene['buf'], descs, validate=False)
    got, status, area = CR.crop_frames(batch, dev(M), valid, 16, return_status=True, antialias=True, return_area=True)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, CR.STATUS_INVALID, CR.STATUS_BAD_DESC, CR.STATUS_BAD_MATRIX, CR.STATUS_BAD_MATRIX, 0]
    assert area.cpu().tolist() == [1, 0, 0, 0, 0, 1]
    got = got.cpu().numpy()
    assert not got[1:5].any() and np.array_equal(got[0], want[1]) and np.array_equal(got[5], want[13])
    M[4, 0] = 2.0 ** -6                                                 # at the bound it is cropped
    status = CR.crop_frames(batch, dev(M), valid, 16, return_status=True, antialias=True)[1]
    assert status.cpu().tolist()[4] == 0


def test_entry_point_refuses_bad_arguments(scene):
    from dir_amd import _capi
    L = _capi.lib()
    batch = batch_of(scene, [0])
    buf = batch.cuda()
    M = dev(np.array([[0.5, 0, 0, 0, 0.5, 0]]))
    out = torch.full((1, 16, 16, 3), 7, dtype=torch.uint8, device='cuda')
    status = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    P = _capi.ptr
    descs = ctypes.c_void_p(buf.data_ptr() + batch._desc_off)

    def call(frames=P(buf), d=descs, m=P(M), B=1, size=16, o=P(out)):
        return L.dir_crop_frames_area(frames, batch.nbytes, d, m, None, B, size, o, P(status), None, _capi.stream_ptr())
    for rc in (call(frames=None), call(d=None), call(m=None), call(o=None), call(B=-1), call(B=CR.MAX_BATCH + 1), call(size=15),
               call(size=CR.MAX_SIZE + 1), call(o=ctypes.c_void_p(out.data_ptr() + 2))):
        assert rc < 0
    torch.cuda.synchronize()
    assert (out == 7).all() and int(status[0]) == -1                    # nothing ran
    assert call() == 0 and call(B=0) == 0
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and np.array_equal(out[0].cpu().numpy(), A.crop_area(scene['frames'][0], [[0.5, 0, 0], [0, 0.5, 0]], 16))
