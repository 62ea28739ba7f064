"""CPU: the host side of the training input (dir_amd.apps.trainset) and the numpy restatements the GPU tests hold the kernels to
(tests/helpers/augment_ref.py), against hand-worked cases and the reference's own label maths (G23, tools/gen_train_aug_golden.py)."""
import os
import sys

import numpy as np
import pytest

from dir_amd.apps import trainset as T

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import augment_ref as R  # noqa: E402


def frame(seed=0):
    return np.random.RandomState(seed).randint(0, 256, (256, 256, 3)).astype(np.uint8)


def g23():
    return dict(np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz')))


def test_identity_warp_returns_the_frame():
    f = frame(1)
    np.testing.assert_array_equal(R.warp_affine_u8(f, T.affine_mat(0.0, 1.0, 0.0, 0.0)[:2]), f)
    sx, sy, fx, fy = T.warp_coords(np.array([1, 0, 0, 0, 1, 0], np.float32), 256, 256)
    assert (fx == 0).all() and (fy == 0).all() and (sx == np.arange(256)[None]).all() and (sy == np.arange(256)[:, None]).all()


@pytest.mark.parametrize('tx,ty', [(3, -2), (-10, 10), (10, 0)])
def test_integer_translation_shifts_with_a_zero_border(tx, ty):
    f = frame(2)
    out = R.warp_affine_u8(f, T.affine_mat(0.0, 1.0, float(tx), float(ty))[:2])
    want = np.zeros_like(f)
    ys, xs = slice(max(ty, 0), 256 + min(ty, 0)), slice(max(tx, 0), 256 + min(tx, 0))
    want[ys, xs] = f[max(-ty, 0):256 - max(ty, 0), max(-tx, 0):256 - max(tx, 0)]
    np.testing.assert_array_equal(out, want)


def test_rotation_by_180_about_the_centre():
    """centre (128, 128): out[y, x] = src[256 - y, 256 - x]; row and column 0 map to 256, outside the frame -> black"""
    f = frame(3)
    M = T.affine_mat(180.0, 1.0, 0.0, 0.0)
    out = R.warp_affine_u8(f, M[:2])
    assert (out[0] == 0).all() and (out[:, 0] == 0).all()
    np.testing.assert_array_equal(out[1:, 1:], f[::-1, ::-1][:255, :255])


def test_bilinear_weights_hand_worked():
    """a half-pixel shift: fx = 16, weights 16384 / 16384; (a + b) / 2 rounded half up by (sum + 2^14) >> 15"""
    f = np.zeros((256, 256), np.uint8)
    f[5, 10], f[5, 11] = 100, 51
    out = R.warp_affine_u8(f, np.array([[1, 0, -0.5], [0, 1, 0]], np.float32))
    assert out[5, 10] == 76                     # (100 + 51) / 2 = 75.5 -> 76
    assert out[5, 11] == 26 and out[5, 9] == 50     # (51 + 0) / 2 = 25.5 -> 26; (0 + 100) / 2 = 50


def test_blur_size_3_angle_0_is_a_horizontal_box():
    k = T.motion_blur_kernel(3, 0.0)
    want = np.zeros((3, 3), np.float32)
    want[1] = np.float32(1) * np.float32(1 / 3)
    np.testing.assert_array_equal(k, want)
    f = frame(4)
    out = R.filter2d_u8(f, k)
    s = f.astype(np.float32)
    pad = np.concatenate([s[:, 1:2], s, s[:, -2:-1]], 1)               # reflect-101 columns
    exp = np.clip(np.rint(((np.float32(0) + k[1, 0] * pad[:, :-2]) + k[1, 1] * pad[:, 1:-1]) + k[1, 2] * pad[:, 2:]), 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(out, exp)


def test_blur_kernels_are_normalised_lines():
    rng = np.random.default_rng(5)
    for size in range(3, 10):
        k = T.motion_blur_kernel(size, rng.uniform(-180, 180) * np.pi / 180)
        assert k.dtype == np.float32 and k.shape == (size, size)
        assert abs(float(k.sum()) - 1) < 1e-5 and (k >= 0).all()


def test_filter2d_reflect101_hand_worked():
    f = np.zeros((256, 256), np.uint8)
    f[0, 1] = 90                                  # reflect-101: column -1 reads column 1
    k = np.zeros((3, 3), np.float32)
    k[1, 0] = 1                                   # out[y, x] = src[y, x - 1]
    out = R.filter2d_u8(f, k)
    assert out[0, 0] == 90 and out[0, 2] == 90 and out[0, 1] == 0


def test_affine_mat_equals_the_reference():
    g = g23()
    for c in range(int(g['cases'])):
        M = T.affine_mat(float(g['rot.%d' % c]), float(g['scale.%d' % c]), float(g['tx.%d' % c]), float(g['ty.%d' % c]))
        assert M.dtype == np.float32
        np.testing.assert_array_equal(M, g['M.%d' % c])


def test_label_maths_against_g23():
    g = g23()
    for c in range(int(g['cases'])):
        p = np.zeros(1, T.AUG_DTYPE)[0]
        p['M'] = g['M.%d' % c][:2].reshape(6)
        p['flip'] = int(g['flip.%d' % c])
        i = lambda k: g['in.' + k]  # noqa: E731
        got = R.augment_labels(i('joint_xyz_left'), i('mesh_xyz_left'), i('joint_xyz_right'), i('mesh_xyz_right'), i('joint_uv_left'),
                               i('mesh_uv_left'), i('joint_uv_right'), i('mesh_uv_right'), i('camera'), p)
        for k, v in got.items():
            ref = g['out.%d.%s' % (c, k)]
            v = v[g['vsub']] if k.startswith('mesh') else v          # G23 keeps every 26th vertex row (and the last)
            assert v.shape == ref.shape
            assert np.abs(v - ref).max() < 1e-9, (c, k)


def test_seg_rule_against_g23():
    g = g23()
    for c in (0, 1):
        np.testing.assert_array_equal(R.seg_of(R.seg_mask(), bool(g['flip.%d' % c]))[0], g['seg.%d' % c][0])


def test_sampler_ranges_and_order():
    rng = np.random.default_rng(0)
    P = T.sample_params(rng, 4000)
    assert P.dtype.itemsize == 400
    a = P['a']
    assert (a >= 0.7).all() and (a <= 1.3).all() and abs(a.mean() - 1.0) < 0.01
    assert (np.abs(P['b']) <= 12.75 + 1e-9).all() and abs(P['b'].mean()) < 0.5
    assert 0.46 < P['flip'].mean() < 0.54
    blur = P['blur'] > 0
    assert 0.27 < blur.mean() < 0.33
    assert set(np.unique(P['blur'][blur])) == set(range(3, 10))
    assert (P['kernel'][~blur] == 0).all()
    # the matrix: scale in 1 +- 0.1 (the norm of a column), the centre moved by at most 10 px per axis
    M = P['M'].reshape(-1, 2, 3).astype(np.float64)
    s = np.hypot(M[:, 0, 0], M[:, 1, 0])
    assert s.min() >= 0.9 - 1e-6 and s.max() <= 1.1 + 1e-6 and s.min() < 0.91 and s.max() > 1.09
    c = np.einsum('nij,j->ni', M, np.array([128.0, 128.0, 1.0])) - 128.0
    assert np.abs(c).max() <= 10 + 1e-3 and np.abs(c).max() > 9.5
    ang = np.degrees(np.arctan2(M[:, 1, 0], M[:, 0, 0]))
    assert ang.min() < -170 and ang.max() > 170
    # same seed -> same draws
    np.testing.assert_array_equal(T.sample_params(np.random.default_rng(7), 16).view(np.uint8),
                                  T.sample_params(np.random.default_rng(7), 16).view(np.uint8))


def test_eval_split_params_are_identity_with_noise():
    P = T.sample_params(np.random.default_rng(1), 64, augment=False)
    assert (P['flip'] == 0).all() and (P['blur'] == 0).all()
    assert (P['M'] == np.array([1, 0, 0, 0, 1, 0], np.float32)).all()
    assert (P['a'] != 0).all() and np.abs(P['b']).max() > 1


def test_restated_sample_matches_hand_composition():
    """the whole image side of one sample with a zero noise field and a = 1, b = 0: the warped frame itself"""
    f, m, d = frame(6), frame(7), frame(8)
    p = np.zeros(1, T.AUG_DTYPE)[0]
    p['M'] = T.affine_mat(30.0, 1.05, 3.0, -4.0)[:2].reshape(6)
    p['flip'] = 1
    p['a'] = 1.0
    out = R.augment_images(f, m, d, p, np.zeros((256, 256, 3), np.float32))
    M = p['M'].reshape(2, 3)
    np.testing.assert_array_equal(out['img_rgb'], R.warp_affine_u8(f[:, ::-1], M).astype(np.float32))
    np.testing.assert_array_equal(out['mask_rgb'], R.warp_affine_u8(m[:, ::-1], M).astype(np.float32))
    assert set(np.unique(out['seg'])) <= {0.0, 1.0, 2.0}
