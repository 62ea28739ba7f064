"""GPU: hand crops from full frames (csrc/crop.hip through dir_amd.utils.crop).

  pixels     crop_frames == tests/helpers/augment_ref.py::warp_affine_u8 byte for byte (integer arithmetic behind IEEE double products) on a
             ragged batch of six frames, five kinds of matrix, crops of 32 and 256 (and of 17, where a lane's four pixels straddle two
             images), and B = 1 against the rows of the batch
  matrices   crop_matrices_from_boxes / crop_matrices_from_meshes == tests/helpers/crop_ref.py bit for bit, every invalid branch, and the
             reference's own matrices (G25) through an identity M_prev
  descriptor a descriptor that reaches past the buffer: a zero crop and a status, the other rows untouched (an argument check: the
             guarded read is never issued)
  mapping    to_frame_pixels / frame_camera against the restatement

Kernel times: tools/bench_crop.py kernels (B = 64, crops of 256, HIP events around 20 direct calls, variants alternating) prints microseconds,
bytes and the share of the copy ceiling per variant; no figures have been taken with it yet."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_ref as R  # noqa: E402
from augment_ref import warp_affine_u8  # noqa: E402

from dir_amd.utils import crop as CR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (256, 256), (300, 200), (64, 640), (1, 1), (128, 96)]            # (H, W); the last one is a view with padded rows
PAD = 10                                                                             # pixels of row padding of the view's parent


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.fixture(scope='module')
def scene():
    """six seeded frames in one packed buffer (the sixth a 128 x 96 view of a 128 x 106 parent: row_stride > 3 W), and per kind of matrix
    one matrix per frame"""
    rng = np.random.default_rng(2500)
    frames = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in SHAPES[:5]]
    parent = rng.integers(0, 256, (SHAPES[5][0], SHAPES[5][1] + PAD, 3)).astype(np.uint8)
    frames.append(parent[:, 3:3 + SHAPES[5][1]])
    chunks, descs, off = [], [], 0
    for f in frames[:5]:
        descs.append((off, f.shape[0], f.shape[1], 3 * f.shape[1]))
        n = -(-f.size // 16) * 16
        chunks.append(np.concatenate([f.reshape(-1), np.zeros(n - f.size, np.uint8)]))
        off += n
    descs.append((off + 9, SHAPES[5][0], SHAPES[5][1], 3 * (SHAPES[5][1] + PAD)))      # the view starts 3 pixels into the parent's first row
    chunks.append(parent.reshape(-1))
    buf = np.concatenate(chunks)
    mats = {
        'translation': [np.array([[1.0, 0, -3.0], [0, 1.0, -2.0]])] * 6,
        'half': [np.array([[0.5, 0, -1.25], [0, 0.5, 2.5]])] * 6,
        'zoom': [np.array([[2.3, 0, -7.7], [0, 2.3, -3.1]])] * 6,
        'outside': [np.array([[1.0, 0, 5000.0], [0, 1.0, 5000.0]])] * 6,
    }
    return {'frames': frames, 'buf': buf, 'descs': descs, 'mats': mats}


def half_outside(frames, size):
    """per frame the crop of a box centred on the frame's corner (0, 0): three quarters of it lie outside"""
    out = []
    for f in frames:
        h, w = f.shape[:2]
        M, ok = R.matrix_from_box([-w / 2, -h / 2, w / 2, h / 2], 1.0, size)
        assert ok == 1
        out.append(M)
    return out


_REF = {}


def reference(scene, kind, size):
    """warp_affine_u8 of every frame, computed once per (kind, size) and shared"""
    if (kind, size) not in _REF:
        mats = half_outside(scene['frames'], size) if kind == 'half_outside' else scene['mats'][kind]
        _REF[kind, size] = (mats, np.stack([warp_affine_u8(f, M, (size, size)) for f, M in zip(scene['frames'], mats)]))
    return _REF[kind, size]


@pytest.mark.parametrize('kind,size', [('translation', 32), ('half', 32), ('zoom', 32), ('half_outside', 32), ('outside', 32),
                                       ('translation', 256), ('half', 256), ('zoom', 17)])
def test_crops_equal_warp_affine_byte_for_byte(scene, kind, size):
    """size 17: 289 pixels per crop, no multiple of the four a lane makes, so lanes straddle two images and the batch ends in byte stores"""
    mats, want = reference(scene, kind, size)
    batch = CR.FrameBatch.from_buffer(scene['buf'], scene['descs'])
    M = dev(np.stack(mats).reshape(6, 6))
    got, status = CR.crop_frames(batch, M, size=size, return_status=True)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (6, size, size, 3) and got.dtype == np.uint8 and not status.cpu().numpy().any()
    for b in range(6):
        bad = (got[b] != want[b]).any(-1)
        assert not bad.any(), (kind, size, b, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if kind == 'outside':
        assert not want.any()
    elif kind == 'half_outside':
        assert all(want[b].any() for b in range(6))
        # the frames at least as large as the crop (scale <= 1): everything left of and above the frame's corner is border
        assert all(not want[b, :size // 2 - 1].any() and not want[b, :, :size // 2 - 1].any() for b in (1, 2, 3))
    else:
        assert want[1].any() and want[3].any()
    # B = 1: every image alone, from a FrameBatch of its own, equals its row of the batch
    for b, f in enumerate(scene['frames']):
        alone = CR.crop_frames(CR.FrameBatch([f]), M[b:b + 1].contiguous(), size=size)
        assert torch.equal(alone[0].cpu(), torch.from_numpy(got[b])), (kind, size, b)


def test_translation_is_a_slice(scene):
    """the hand-worked case of tests/test_crop_ref.py on the GPU: box (70, 40) - (326, 296) at ratio 1 -> canvas[40:296, 70:326]"""
    canvas = np.random.default_rng(25).integers(0, 256, (400, 500, 3)).astype(np.uint8)
    M, valid = CR.crop_matrices_from_boxes(dev(np.float32([[70, 40, 326, 296]])), ratio=1.0, size=256)
    got = CR.crop_frames(CR.FrameBatch([canvas]), M, valid, 256)
    assert np.array_equal(M.cpu().numpy(), [[1, 0, -70, 0, 1, -40]]) and int(valid[0]) == 1
    assert np.array_equal(got[0].cpu().numpy(), canvas[40:296, 70:326])


def test_invalid_rows_are_black(scene):
    batch = CR.FrameBatch.from_buffer(scene['buf'], scene['descs'])
    mats, want = reference(scene, 'translation', 32)
    M = np.stack(mats).reshape(6, 6).copy()
    M[2] = [np.nan, 0, 0, 0, 1, 0]                                      # not finite
    M[3] = [1e-9, 0, 0, 0, 1e-9, 0]                                     # a source coordinate of 3.1e10 px
    valid = dev(np.int32([1, 0, 1, 1, 1, 1]))
    got, status = CR.crop_frames(batch, dev(M), valid, 32, return_status=True)
    assert status.cpu().tolist() == [0, CR.STATUS_INVALID, CR.STATUS_BAD_MATRIX, CR.STATUS_BAD_MATRIX, 0, 0]
    got = got.cpu().numpy()
    assert not got[1:4].any() and all(np.array_equal(got[b], want[b]) for b in (0, 4, 5))


def test_descriptor_past_the_buffer_is_refused(scene):
    """an argument check, not a fault: the kernel compares the descriptor with the buffer's length first and issues no read for the image"""
    mats, want = reference(scene, 'translation', 32)
    n = scene['buf'].size
    descs = list(scene['descs'])
    descs[1] = (descs[1][0], 256, 256, n)                                # its second row would start past the end
    descs[2] = (n - 100, 300, 200, 600)                                  # begins inside, ends 180 000 bytes past the end
    descs[4] = (-16, 1, 1, 3)                                            # begins before the buffer
    with pytest.raises(ValueError):
        CR.FrameBatch.from_buffer(scene['buf'], descs)
    batch = CR.FrameBatch.from_buffer(scene['buf'], descs, validate=False)
    got, status = CR.crop_frames(batch, dev(np.stack(mats).reshape(6, 6)), size=32, return_status=True)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, CR.STATUS_BAD_DESC, CR.STATUS_BAD_DESC, 0, CR.STATUS_BAD_DESC, 0]
    got = got.cpu().numpy()
    assert not got[[1, 2, 4]].any() and all(np.array_equal(got[b], want[b]) for b in (0, 3, 5))


def seeded_boxes(B, seed):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(-50, 1500, B), rng.uniform(-50, 900, B)
    return np.stack([x0, y0, x0 + rng.uniform(30, 600, B), y0 + rng.uniform(30, 600, B)], 1).astype(np.float32)


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('ratio,size', [(0.8, 256), (0.7, 32)])
def test_box_matrices_bit_for_bit(B, ratio, size):
    boxes = seeded_boxes(B, 100 + B)
    M, valid = CR.crop_matrices_from_boxes(dev(boxes), ratio, size)
    M, valid = M.cpu().numpy(), valid.cpu().numpy()
    for b in range(B):
        want, ok = R.matrix_from_box(boxes[b], ratio, size)
        assert ok == 1 == valid[b] and np.array_equal(bits(M[b]), bits(want.reshape(-1))), b


def test_box_matrices_invalid_branches():
    boxes = np.float32([[10, 20, 110, 90], [np.nan, 20, 110, 90], [10, 20, np.inf, 90], [10, 20, 10, 20], [10, 20, 10.5, 20.5],
                        [0, 0, 30000, 100], [2.0 ** 20, 0, 2.0 ** 20 + 200, 100], [110, 90, 10, 20], [0, 0, 3, 3], [0, 0, 3.3, 3.3]])
    M, valid = CR.crop_matrices_from_boxes(dev(boxes), 0.8, 256)
    M, valid = M.cpu().numpy(), valid.cpu().numpy()
    want = [R.matrix_from_box(b, 0.8, 256) for b in boxes]
    assert valid.tolist() == [w[1] for w in want] == [1, 0, 0, 0, 0, 0, 0, 1, 0, 1]     # corners in any order; a 3 px box needs s = 68.3, a 3.3 px one 62.1
    for b in range(len(boxes)):
        assert np.array_equal(bits(M[b]), bits(want[b][0].reshape(-1))), b
    assert np.array_equal(bits(M[7]), bits(M[0])) and not M[valid == 0].any()


def seeded_stage(B, seed):
    """hand-sized vertices (+-0.1 m), s in 3..8, small t; M_prev a plausible crop of a large frame"""
    rng = np.random.default_rng(seed)
    st = {'pd_mesh_xyz_left': rng.uniform(-0.1, 0.1, (B, 778, 3)), 'pd_mesh_xyz_right': rng.uniform(-0.1, 0.1, (B, 778, 3)),
          'pd_proj_left': np.concatenate([rng.uniform(3, 8, (B, 1)), rng.uniform(-0.3, 0.3, (B, 2))], 1),
          'pd_proj_right': np.concatenate([rng.uniform(3, 8, (B, 1)), rng.uniform(-0.3, 0.3, (B, 2))], 1)}
    s = rng.uniform(0.2, 3.0, B)
    M_prev = np.stack([s, np.zeros(B), rng.uniform(-900, 100, B), np.zeros(B), s, rng.uniform(-900, 100, B)], 1)
    return {k: v.astype(np.float32) for k, v in st.items()}, M_prev


def host_chain(st, M_prev, ratio, size):
    return [R.matrix_from_meshes(st['pd_mesh_xyz_left'][b], st['pd_mesh_xyz_right'][b], st['pd_proj_left'][b], st['pd_proj_right'][b],
                                 M_prev[b], ratio, size) for b in range(len(M_prev))]


@pytest.mark.parametrize('B', [1, 5])
def test_mesh_matrices_bit_for_bit(B):
    st, M_prev = seeded_stage(B, 200 + B)
    M, valid = CR.crop_matrices_from_meshes({k: dev(v) for k, v in st.items()}, dev(M_prev), 0.8, 256)
    M, valid = M.cpu().numpy(), valid.cpu().numpy()
    for b, (want, ok) in enumerate(host_chain(st, M_prev, 0.8, 256)):
        assert ok == 1 == valid[b] and np.array_equal(bits(M[b]), bits(want.reshape(-1))), b
    # the same sample gives the same bits alone and in a batch
    if B == 5:
        one = CR.crop_matrices_from_meshes({k: dev(v[3:4]) for k, v in st.items()}, dev(M_prev[3:4]), 0.8, 256)[0]
        assert np.array_equal(bits(one.cpu().numpy()[0]), bits(M[3]))


def test_mesh_matrices_invalid_branches_hold_the_previous_box():
    st, M_prev = seeded_stage(9, 300)
    st['pd_mesh_xyz_left'][1, 100, 1] = np.nan                          # a non-finite vertex
    st['pd_proj_right'][2, 0] = np.inf                                  # a non-finite camera
    st['pd_proj_left'][3] = st['pd_proj_right'][3] = 0                  # every vertex on one point: L = 0
    st['pd_proj_left'][4, 0] = st['pd_proj_right'][4, 0] = 1e-3         # a collapsed prediction: s > 64
    st['pd_proj_left'][4, 1:] = st['pd_proj_right'][4, 1:]
    st['pd_proj_left'][5, 0] = 2000.0                                   # an exploded one: s < 2^-6
    M_prev[6] = [1e-3, 0, -1000.0, 0, 1e-3, 3.0]                         # a corner beyond 2^20 px (s stays inside its range at ratio 0.8)
    st['pd_proj_left'][6, 0] = st['pd_proj_right'][6, 0] = 0.04
    st['pd_proj_left'][6, 1:] = st['pd_proj_right'][6, 1:] = 0
    M_prev[7] = 0                                                       # a previous box that was itself invalid (zeros): division by zero
    want = host_chain(st, M_prev, 0.8, 256)
    assert [w[1] for w in want] == [1, 0, 0, 0, 0, 0, 0, 0, 1]
    M, valid = CR.crop_matrices_from_meshes({k: dev(v) for k, v in st.items()}, dev(M_prev), 0.8, 256)
    M, valid = M.cpu().numpy(), valid.cpu().numpy()
    assert valid.tolist() == [w[1] for w in want]
    for b in range(9):
        assert np.array_equal(bits(M[b]), bits(want[b][0].reshape(-1))), b
        if not valid[b]:
            assert np.array_equal(bits(M[b]), bits(M_prev[b])), b
    # row 6 is invalid because of the coordinate bound alone
    pts = [R.frame_points(st['pd_mesh_xyz_' + s][6], st['pd_proj_' + s][6], M_prev[6]) for s in ('left', 'right')]
    lo, hi = np.min([p.min(0) for p in pts], 0), np.max([p.max(0) for p in pts], 0)
    L = (hi - lo).max() / 2 / 0.8
    assert R.MIN_SCALE <= 128 / L <= R.MAX_SCALE and np.abs(np.concatenate([(lo + hi) / 2 - L, (lo + hi) / 2 + L])).max() > R.MAX_COORD


def test_mesh_matrices_reproduce_the_reference_through_an_identity_crop(golden):
    """G25's float64 labels as a prediction: with pd_proj = (1, 0, 0) the projection is uv = xy exactly, and with M_prev the identity the
    frame position is (uv + 1) * 128, so vertices xy = float32(label / 128 - 1) put the points on the labels rounded to float32's grid
    in uv.  On those points the kernel equals the restatement bit for bit; G25's own matrix (from the unrounded labels) is met to that
    rounding: a point moves by at most e = 128 * ulp32(max |uv|) / 2, so L by e / ratio, s by s * (e / ratio) / L, and
    t = s (L - mid) by |ds| |L - mid| + s (e / ratio + e); the gate is twice that first-order bound."""
    g = golden('g25_crop')
    ident = np.array([[1.0, 0, 0, 0, 1.0, 0]])
    for c in range(len(g['seed'])):
        ratio, size = float(g['ratio'][c]), int(g['size'][c])
        pts, _ = R.make_case(int(g['seed'][c]))
        xy = [(p / (size / 2) - 1).astype(np.float32) for p in pts]
        st = {'pd_mesh_xyz_left': np.concatenate([xy[0], np.zeros((778, 1), np.float32)], 1)[None],
              'pd_mesh_xyz_right': np.concatenate([xy[1], np.zeros((778, 1), np.float32)], 1)[None],
              'pd_proj_left': np.float32([[1, 0, 0]]), 'pd_proj_right': np.float32([[1, 0, 0]])}
        M, valid = CR.crop_matrices_from_meshes({k: dev(v) for k, v in st.items()}, dev(ident), ratio, size)
        M = M.cpu().numpy()[0]
        want, ok = R.matrix_from_points([(x.astype(np.float64) + 1) * (size / 2) for x in xy], ratio, size)
        assert ok == 1 == int(valid[0]) and np.array_equal(bits(M), bits(want.reshape(-1))), c
        ref = g['matrix'][c]
        e = (size / 2) * float(np.spacing(np.float32(max(np.abs(x).max() for x in xy)))) / 2
        s = ref[0, 0]
        L = (size / 2) / s
        ds = s * (e / ratio) / L
        dt = ds * np.abs(ref[:, 2] / s).max() + s * (e / ratio + e)
        assert abs(M[0] - s) <= 2 * ds and abs(M[4] - s) <= 2 * ds and np.abs(M[[2, 5]] - ref[:, 2]).max() <= 2 * dt, c
        assert ds < 1e-5 * s and dt < 1e-2                                # the gate bites: a hundredth of a pixel; a wrong ratio or centre costs pixels


def test_pixel_mapping():
    # the translation case is exact: uv on the crop's pixel grid, an integer offset
    M = dev(np.array([[1.0, 0, -70, 0, 1.0, -40], [1.0, 0, 3, 0, 1.0, -1000]]))
    k = np.random.default_rng(7).integers(0, 257, (2, 21, 2))
    uv = (k / 128.0 - 1).astype(np.float32)
    got = CR.to_frame_pixels(dev(uv), M).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got[0], k[0] + np.float32([70, 40])) and np.array_equal(got[1], k[1] + np.float32([-3, 1000]))
    sc, tr = CR.frame_camera(dev(np.float32([[2, 0, 0], [0.5, -1, 1]])), M)
    assert sc.cpu().tolist() == [256.0, 64.0] and np.array_equal(tr.cpu().numpy(), np.float32([[198, 168], [-3, 1256]]))
    # elsewhere: within 2 float32 ulps of the largest coordinate, against the restatement rounded to float32
    st, Mp = seeded_stage(5, 400)
    uv = np.random.default_rng(8).uniform(-1.2, 1.2, (5, 21, 2)).astype(np.float32)
    got = CR.to_frame_pixels(dev(uv), dev(Mp)).cpu().numpy()
    want = np.stack([R.to_frame_pixels(uv[b], Mp[b]) for b in range(5)])
    gate = 2 * float(np.spacing(np.float32(np.abs(want).max())))
    assert np.abs(got.astype(np.float64) - want.astype(np.float32)).max() <= gate and np.abs(want).max() > 100
    sc, tr = CR.frame_camera(dev(st['pd_proj_left']), dev(Mp))
    ws, wt = zip(*[R.frame_camera(st['pd_proj_left'][b], Mp[b]) for b in range(5)])
    gate = 2 * float(np.spacing(np.float32(max(np.abs(ws).max(), np.abs(wt).max()))))
    assert np.abs(sc.cpu().numpy().astype(np.float64) - np.float32(ws)).max() <= gate
    assert np.abs(tr.cpu().numpy().astype(np.float64) - np.float32(wt)).max() <= gate
    # the camera and the points agree: frame pixel of a vertex = scale_px * xy + trans_px
    xy = st['pd_mesh_xyz_left'][:, :50, :2]
    proj = st['pd_proj_left']
    uvv = (proj[:, None, :1] * xy + proj[:, None, 1:]).astype(np.float32)
    px = np.stack([R.to_frame_pixels(uvv[b], Mp[b]) for b in range(5)])
    assert np.abs(np.float64(ws)[:, None, None] * xy + np.float64(wt)[:, None] - px).max() < 1e-3
