"""CPU: the float64 restatement of the crop rules (tests/helpers/crop_ref.py) against the reference's own cut_img (G25:
tests/golden/g25_crop.npz, written by tools/gen_crop_golden.py), a hand-worked case, the invalid branches, and the host side of
dir_amd.utils.crop and of the three entry points (argument checks that launch nothing).

Equality with G25 is to the bit: the operation order is the reference's and every operation is a correctly rounded IEEE double one."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_ref as R  # noqa: E402
from augment_ref import warp_affine_u8  # noqa: E402


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def g25_cases(golden):
    g = golden('g25_crop')
    n = len(g['seed'])
    assert n >= 16
    for c in range(n):
        pts, K = R.make_case(int(g['seed'][c]))
        assert R.checksum(pts, K) == g['checksum'][c], c                   # the generator has not drifted
        yield c, g, pts, K, float(g['ratio'][c]), int(g['size'][c])


def test_matrices_equal_the_reference_bit_for_bit(golden):
    seen = set()
    for c, g, pts, K, ratio, size in g25_cases(golden):
        M, ok = R.matrix_from_points(pts, ratio, size)
        assert ok == 1 and np.array_equal(bits(M), bits(g['matrix'][c])), c
        seen.add((ratio, size))
    assert {(0.8, 256), (0.7, 256), (1.0, 256), (0.8, 32)} <= seen


def test_labels_and_intrinsics_equal_the_reference_bit_for_bit(golden):
    for c, g, pts, K, ratio, size in g25_cases(golden):
        M = g['matrix'][c]
        got = np.stack([R.transform_labels(p, M) for p in pts])[:, ::R.LABEL_STEP]
        assert np.array_equal(bits(got), bits(g['labels'][c])), c
        assert np.array_equal(bits(R.transform_camera(K, M)), bits(g['camera'][c])), c
        # every label lands inside the crop, the extreme ones `ratio` of the way from its centre to its edge
        inside = np.concatenate([R.transform_labels(p, M) for p in pts])
        assert inside.min() > -1e-9 and inside.max() < size + 1e-9             # ratio 1: the extreme labels sit on the crop's edge, to rounding
        assert abs((inside.max(0) - inside.min(0)).max() / size - ratio) < 1e-12


def test_hand_worked_translation():
    """points spanning (70, 40) - (326, 296), ratio 1, size 256: mid = (198, 168), L = 128, s = 1, M = [[1, 0, -70], [0, 1, -40]] exactly
    (checked against the reference's cut_img when this was written); the warp with it is a plain slice"""
    pts = [np.array([[70.0, 40.0], [200.0, 100.0]]), np.array([[326.0, 296.0], [100.0, 250.0]])]
    M, ok = R.matrix_from_points(pts, 1.0, 256)
    assert ok == 1 and np.array_equal(bits(M), bits([[1.0, 0.0, -70.0], [0.0, 1.0, -40.0]]))
    Mb, okb = R.matrix_from_box([70, 40, 326, 296], 1.0, 256)
    assert okb == 1 and np.array_equal(bits(Mb), bits(M))
    canvas = np.random.default_rng(25).integers(0, 256, (400, 500, 3)).astype(np.uint8)
    assert np.array_equal(warp_affine_u8(canvas, M, (256, 256)), canvas[40:296, 70:326])
    # and back: crop pixel (0, 0) is frame pixel (70, 40); the crop's uv = -1 is its position 0
    assert np.array_equal(R.to_frame_pixels(np.array([[-1.0, -1.0], [0.0, 0.0]]), M), [[70.0, 40.0], [198.0, 168.0]])
    sc, tr = R.frame_camera(np.array([2.0, 0.0, 0.0]), M)
    assert sc == 256.0 and np.array_equal(tr, [198.0, 168.0])


def test_invalid_inputs():
    ok_box = [10.0, 20.0, 110.0, 90.0]
    assert R.matrix_from_box(ok_box)[1] == 1
    for box in ([np.nan, 20, 110, 90], [10, 20, np.inf, 90], [10, 20, 10, 20],          # not finite; zero area
                [10, 20, 10.5, 20.5],                                                    # s = 128 / (0.25 / 0.8) = 409.6 > 64
                [0, 0, 30000, 100],                                                      # s = 128 / 18750 < 2^-6
                [2.0 ** 20, 0, 2.0 ** 20 + 200, 100]):                                   # a crop corner beyond 2^20
        M, ok = R.matrix_from_box(box)
        assert ok == 0 and not M.any(), box
    # the scale's range is closed at both ends: L = 2 gives exactly 64, L = 8192 exactly 2^-6
    assert R.matrix_from_box([0, 0, 4, 4], 1.0, 256)[1] == 1 and R.matrix_from_box([0, 0, 3.99, 3.99], 1.0, 256)[1] == 0
    assert R.matrix_from_box([0, 0, 16384, 100], 1.0, 256)[1] == 1 and R.matrix_from_box([0, 0, 16400, 100], 1.0, 256)[1] == 0
    # tracking: an invalid result holds the previous matrix
    prev = np.array([[0.5, 0, -10.0], [0, 0.5, -20.0]])
    mesh = np.random.default_rng(1).uniform(-0.1, 0.1, (778, 3)).astype(np.float32)
    M, ok = R.matrix_from_meshes(mesh, mesh, np.float32([5, 0, 0]), np.float32([5, 0.1, 0]), prev)
    assert ok == 1 and M[0, 0] != 0.5
    for proj in (np.float32([np.nan, 0, 0]), np.float32([1e-6, 0, 0]), np.float32([0, 0, 0])):      # not finite; s > 64; zero area
        M, ok = R.matrix_from_meshes(mesh, mesh, proj, proj, prev)
        assert ok == 0 and np.array_equal(M, prev)


def test_tracking_chain_is_the_identity_on_a_perfect_prediction():
    """a prediction whose projection fills `ratio` of the crop, chained through any M_prev, gives back M_prev up to rounding"""
    rng = np.random.default_rng(3)
    mesh = rng.uniform(-0.1, 0.1, (778, 3)).astype(np.float32)
    mesh[0, :2], mesh[1, :2] = (-0.1, -0.1), (0.1, 0.1)
    proj = np.float32([8.0, 0.0, 0.0])                                      # uv in -0.8 .. 0.8
    prev = np.array([[0.37, 0, -51.25], [0, 0.37, 13.5]])
    M, ok = R.matrix_from_meshes(mesh, mesh, proj, proj, prev, 0.8, 256)
    assert ok == 1 and np.abs(M - prev).max() < 1e-5


def test_entry_points_check_their_arguments_before_any_launch():
    import torch  # noqa: F401
    from dir_amd import _capi
    L = _capi.lib()
    one = ctypes.c_void_p(16)

    def bad(rc, word):
        assert rc == -1 and word in L.dir_last_error(), (rc, L.dir_last_error())
    assert L.dir_crop_matrices_from_boxes(None, 0, 0.8, 256, None, None, None) == 0                 # an empty batch is a no-op
    bad(L.dir_crop_matrices_from_boxes(None, 1, 0.8, 256, one, one, None), b'null pointer')
    bad(L.dir_crop_matrices_from_boxes(one, 1, 0.0, 256, one, one, None), b'ratio')
    bad(L.dir_crop_matrices_from_boxes(one, 1, float('nan'), 256, one, one, None), b'ratio')
    bad(L.dir_crop_matrices_from_boxes(one, 1, 0.8, 8, one, one, None), b'size')
    bad(L.dir_crop_matrices_from_boxes(one, 5000, 0.8, 256, one, one, None), b'B 5000')
    bad(L.dir_crop_matrices_from_meshes(one, one, one, None, one, 1, 0.8, 256, one, one, None), b'null pointer')
    bad(L.dir_crop_matrices_from_meshes(one, one, one, one, one, 1, 0.8, 2048, one, one, None), b'size')
    assert L.dir_crop_frames(None, 0, None, None, None, 0, 256, None, None, None) == 0
    bad(L.dir_crop_frames(one, 16, one, None, None, 1, 256, one, None, None), b'null pointer')
    bad(L.dir_crop_frames(one, 0, one, one, None, 1, 256, one, None, None), b'bytes')
    bad(L.dir_crop_frames(one, 16, one, one, None, 1, 15, one, None, None), b'size')
    bad(L.dir_crop_frames(one, 16, one, one, None, 1, 256, ctypes.c_void_p(18), None, None), b'aligned')
    assert ctypes.sizeof(_capi.FrameDesc) == 24


def test_frame_batch_packs_and_validates_on_the_host():
    from dir_amd.utils import crop as CR
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((5, 7), (1, 1), (16, 3))]
    fb = CR.FrameBatch(frames + [frames[0][:, ::-1]])                      # a view that is not contiguous is copied
    assert len(fb) == 4 and fb.sizes == [(5, 7), (1, 1), (16, 3), (5, 7)]
    for f, (off, h, w, stride) in zip(frames + [frames[0][:, ::-1]], fb.descs):
        assert off % CR.FRAME_ALIGN == 0 and stride == 3 * w
        assert np.array_equal(fb.buffer[off:off + h * stride].reshape(h, w, 3), f)
    assert fb.nbytes <= len(fb.buffer)
    with pytest.raises(ValueError):
        CR.FrameBatch([])
    with pytest.raises(ValueError):
        CR.FrameBatch([np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        CR.FrameBatch([np.zeros((4, 4, 3), np.float32)])
    assert len(CR.FrameBatch([np.zeros((1, CR.MAX_SIDE, 3), np.uint8)])) == 1
    with pytest.raises(ValueError):                                         # wider than the kernel's descriptor rule allows: refused here,
        CR.FrameBatch([frames[0], np.zeros((1, CR.MAX_SIDE + 1, 3), np.uint8)])      # not answered with a black crop later
    buf = np.zeros(1000, np.uint8)
    assert len(CR.FrameBatch.from_buffer(buf, [(0, 10, 10, 100)])) == 1     # 9 * 100 + 30 = 930 <= 1000
    for d in ((0, 11, 10, 100), (-1, 2, 2, 6), (0, 2, 2, 5), (0, 0, 2, 6), (990, 1, 4, 12)):
        with pytest.raises(ValueError):
            CR.FrameBatch.from_buffer(buf, [d])
    assert len(CR.FrameBatch.from_buffer(buf, [(0, 11, 10, 100)], validate=False)) == 1


def test_predict_lists_images_in_natural_order(tmp_path):
    from dir_amd.apps import predict as P
    for n in ('f10.png', 'f2.png', 'f1.jpg', 'note.txt', 'F3.JPEG'):
        (tmp_path / n).write_bytes(b'')
    assert [os.path.basename(p) for p in P.list_images([str(tmp_path)])] == ['f1.jpg', 'f2.png', 'F3.JPEG', 'f10.png']
    assert P.list_images([str(tmp_path / 'f10.png'), str(tmp_path / 'f2.png')]) == [str(tmp_path / 'f2.png'), str(tmp_path / 'f10.png')]
    (tmp_path / 'b').mkdir()
    (tmp_path / 'a').mkdir()
    (tmp_path / 'a' / '1.png').write_bytes(b'')
    (tmp_path / 'b' / '1.png').write_bytes(b'')
    (tmp_path / 'b' / '0.png').write_bytes(b'')
    seqs = P.list_sequences([str(tmp_path)])
    assert [[os.path.basename(p) for p in s] for s in seqs] == [['1.png'], ['0.png', '1.png']]


def test_predict_tracks_at_most_bs_sequences_at_a_time_and_keys_boxes_by_sequence(tmp_path):
    from dir_amd.apps import predict as P
    seqs = [['a0', 'a1'], ['b0', 'b1', 'b2'], ['c0'], ['d0', 'd1'], ['e0']]
    groups = P.lockstep_groups(seqs, 2)
    assert groups == [[[(1, 'b0'), (0, 'a0')], [(1, 'b1'), (0, 'a1')], [(1, 'b2')]], [[(3, 'd0'), (2, 'c0')], [(3, 'd1')]], [[(4, 'e0')]]]
    assert all(len(st) <= 2 for g in groups for st in g) and sorted(x for g in groups for st in g for _, x in st) == sorted(sum(seqs, []))
    assert P.lockstep_groups(seqs, 8) == [P.lockstep(seqs)]
    boxes = {'a/0.png': [1, 2, 3, 4], 'b/0': [5, 6, 7, 8], '0.png': [9, 9, 9, 9], '1': [0, 0, 1, 1]}
    assert P.box_for(boxes, str(tmp_path / 'a' / '0.png'), 10, 20) == [1.0, 2.0, 3.0, 4.0]
    assert P.box_for(boxes, str(tmp_path / 'b' / '0.png'), 10, 20) == [5.0, 6.0, 7.0, 8.0]
    assert P.box_for(boxes, str(tmp_path / 'c' / '0.png'), 10, 20) == [9.0, 9.0, 9.0, 9.0]
    assert P.box_for(boxes, str(tmp_path / 'c' / '1.jpg'), 10, 20) == [0.0, 0.0, 1.0, 1.0]
    assert P.box_for(boxes, str(tmp_path / 'c' / '2.jpg'), 10, 20) == [0.0, 0.0, 19.0, 9.0]
