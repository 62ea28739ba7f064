"""CPU: the restatement of the anti-aliased crop (tests/helpers/crop_area_ref.py).

  Pillow pin     resample_box == PIL.Image.resize((n, n), BILINEAR, box=box) byte for byte wherever Pillow's window lies inside the frame it
                 is given (frames padded with zeros by the test included): 2, 4, 1 / 0.3, 7.3 and 64 / 3 source pixels per output pixel,
                 n = 16 and 17.  Pillow reads the box as float32, so every box here is float32-exact
  closed forms   a constant frame stays constant inside and fades by the inside weight share at the border (the zero border keeps its
                 weight); 2 px stripes at 4 px per output pixel become 127 / 128 where the plain warp gives 0 or 255
  box            box_from_matrix on dyadic matrices against edges worked by hand
  selection      s = 1, s > 1, a rotation, a mirror: crop_area is warp_affine_u8
  C ABI          dir_crop_frames_area checks its arguments before any launch"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_area_ref as A  # noqa: E402
from augment_ref import warp_affine_u8  # noqa: E402

F32 = np.float32
SCALES = [2.0, 4.0, float(F32(1 / 0.3)), float(F32(7.3)), float(F32(64 / 3))]          # source pixels per output pixel


def f32_box(x0, y0, scale, n):
    """a float32-exact box of n * scale source pixels a side from (x0, y0), a multiple of 1/64: dyadic scales give exact far corners
    already; the others are rounded to float32 HERE, and both sides get the rounded values.  Pillow also subtracts the edges in float32
    (precompute_coeffs: in1 - in0 on floats) where the rule subtracts in double; from a corner on the 1/64 grid the float32 difference is
    exact, so the two agree -- asserted, because a box whose width float32 rounds is outside what Pillow can pin"""
    assert x0 * 64 == int(x0 * 64) and y0 * 64 == int(y0 * 64)
    box = tuple(float(F32(v)) for v in (x0, y0, x0 + n * scale, y0 + n * scale))
    assert float(F32(box[2]) - F32(box[0])) == box[2] - box[0] and float(F32(box[3]) - F32(box[1])) == box[3] - box[1]
    return box


def pillow_resize(frame, box, n):
    Image = pytest.importorskip('PIL.Image')
    bil = getattr(Image, 'Resampling', Image).BILINEAR
    return np.asarray(Image.fromarray(frame).resize((n, n), bil, box=box))


def window_inside(box, n, h, w):
    """Pillow clamps a window to the image; the pin is only over boxes where it has nothing to clamp"""
    for in0, in1, lim in ((box[0], box[2], w), (box[1], box[3], h)):
        co = A.coefficients(in0, in1, n)
        if co[0][0] < 0 or co[-1][0] + len(co[-1][1]) > lim:
            return False
    return True


@pytest.mark.parametrize('n', [16, 17])
@pytest.mark.parametrize('scale', SCALES)
def test_resample_box_equals_pillow_byte_for_byte(scale, n):
    rng = np.random.default_rng(int(scale * 1000) + n)
    for trial in range(3):
        x0, y0 = (float(rng.integers(0, 640)) / 64 + np.ceil(scale) for _ in range(2))  # multiples of 1/64, a support away from the edge
        box = f32_box(x0, y0, scale, n)
        h, w = int(box[3] + scale) + 3 + trial, int(box[2] + scale) + 2 + 2 * trial
        frame = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        assert window_inside(box, n, h, w)
        got, want = A.resample_box(frame, box, n), pillow_resize(frame, box, n)
        bad = (got != want).any(-1)
        assert not bad.any(), (scale, n, trial, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize('scale,n', [(4.0, 16), (float(F32(7.3)), 17)])
def test_zero_border_equals_pillow_on_a_frame_padded_with_zeros(scale, n):
    """a box that reaches past all four sides of a small frame: Pillow on the frame padded with zeros (a frame in its own right)
    == resample_box on the padded frame == resample_box on the small frame with the box moved: the taps outside read 0 and keep their weight"""
    rng = np.random.default_rng(n)
    pad = int(3 * scale) + 8
    side = int(n * scale) - int(2 * scale)
    small = rng.integers(1, 256, (side, side - 3, 3)).astype(np.uint8)
    padded = np.zeros((side + 2 * pad, side - 3 + 2 * pad, 3), np.uint8)
    padded[pad:pad + side, pad:pad + side - 3] = small
    box = f32_box(pad - np.floor(80 * scale) / 64, pad - np.floor(48 * scale) / 64, scale, n)
    assert window_inside(box, n, *padded.shape[:2])
    want = pillow_resize(padded, box, n)
    assert np.array_equal(A.resample_box(padded, box, n), want)
    moved = tuple(v - pad for v in box)                                                  # an integer shift: exact
    assert moved[0] < 0 and moved[1] < 0 and moved[2] > side - 3 and moved[3] > side
    assert np.array_equal(A.resample_box(small, moved, n), want)
    assert want[0].max() < want[n // 2].max()                                            # the border really fades


def test_constant_frame_fades_by_the_inside_weight_share():
    n, scale = 16, 4.0
    frame = np.full((80, 80, 3), 255, np.uint8)
    inside = A.resample_box(frame, (6.0, 10.0, 6.0 + n * scale, 10.0 + n * scale), n)
    assert (inside == 255).all()
    box = (-10.0, 8.0, -10.0 + n * scale, 8.0 + n * scale)                               # the left columns hang over the frame's left edge
    got = A.resample_box(frame, box, n)
    shares = []
    for u, (xmin, K) in enumerate(A.coefficients(box[0], box[2], n)):
        k_in = sum(k for j, k in enumerate(K) if 0 <= xmin + j < 80)
        want = min(255, (2 ** 21 + 255 * k_in) >> 22)
        assert (got[:, u] == want).all(), (u, want, got[:, u].reshape(-1)[:6].tolist())
        shares.append(k_in / 2 ** 22)
    assert shares[0] == 0 and 0 < shares[2] < 1 and abs(shares[-1] - 1) < 1e-5           # outside, straddling (10 / 4 = 2.5), inside
    assert got[0, 2, 0] == round(255 * shares[2])


def test_stripes_alias_under_the_plain_warp_and_average_under_the_area_rule():
    n = 16
    frame = np.zeros((96, 96, 3), np.uint8)
    frame[:, 1::2] = 255                                                                 # period 2 px
    M = np.array([[0.25, 0, -2.0], [0, 0.25, -2.0]])                                     # exactly 4 source px per output px
    assert A.is_shrinking(M)
    got = A.crop_area(frame, M, n)
    assert set(np.unique(got[1:-1, 1:-1]).tolist()) <= {127, 128}
    plain = warp_affine_u8(frame, M, (n, n))
    assert set(np.unique(plain[1:-1, 1:-1]).tolist()) & {0, 255}                         # every sample lands on one phase of the stripes


def test_box_from_matrix_on_dyadic_matrices():
    assert A.box_from_matrix([[1.0, 0, 0], [0, 1.0, 0]], 16) == (0.0, 0.0, 16.0, 16.0)
    # x: 0.5 - (-1.25 + 0.5) / 0.5 = 2, + 16 / 0.5 = 34;  y: 0.5 - (2.5 + 0.5) / 0.25 = -11.5, + 16 / 0.25 = 52.5
    assert A.box_from_matrix([[0.5, 0, -1.25], [0, 0.25, 2.5]], 16) == (2.0, -11.5, 34.0, 52.5)
    # 1/64: 0.5 - (3 + 0.5) * 64 = -223.5, + 17 * 64 = 864.5
    assert A.box_from_matrix([[2.0 ** -6, 0, 3.0], [0, 2.0 ** -6, 3.0]], 17) == (-223.5, -223.5, 864.5, 864.5)
    # the centre of crop pixel u is frame position (u - t) / s in warpAffine's terms: box edge + (u + 0.5) / s - 0.5
    x0, _, x1, _ = A.box_from_matrix([[0.25, 0, -5.0], [0, 0.25, 0]], 16)
    assert x0 + (3 + 0.5) * 4 - 0.5 == (3 + 5.0) / 0.25 and x1 - x0 == 64


def test_rule_selection():
    rng = np.random.default_rng(4)
    frame = rng.integers(0, 256, (60, 70, 3)).astype(np.uint8)
    c, s = np.cos(0.3), np.sin(0.3)
    others = {'s = 1': [[1.0, 0, -3.0], [0, 1.0, -2.0]], 's > 1': [[1.7, 0, -7.0], [0, 1.7, 1.0]],
              'rotation': [[0.5 * c, 0.5 * s, 4.0], [-0.5 * s, 0.5 * c, 9.0]], 'mirror': [[-0.5, 0, 30.0], [0, 0.5, 0.0]],
              'shear': [[0.5, 0.1, 0.0], [0, 0.5, 0.0]]}
    for name, M in others.items():
        assert not A.is_shrinking(M), name
        assert np.array_equal(A.crop_area(frame, M, 16), warp_affine_u8(frame, np.array(M), (16, 16))), name
    assert A.is_shrinking([[0.5, 0, 0], [0, 0.5, 0]]) and A.is_shrinking([[0.5, 0, 0], [0, 2.0, 0]]) and A.is_shrinking([[1.0, 0, 0], [0, 0.99, 0]])
    assert not A.is_shrinking([[np.nan, 0, 0], [0, 0.5, 0]])
    M = [[0.3, 0, 1.0], [0, 0.3, -2.0]]
    assert np.array_equal(A.crop_area(frame, M, 17), A.resample_box(frame, A.box_from_matrix(M, 17), 17))
    assert not np.array_equal(A.crop_area(frame, M, 17), warp_affine_u8(frame, np.array(M), (17, 17)))


def test_entry_point_checks_its_arguments_before_any_launch():
    import torch  # noqa: F401
    from dir_amd import _capi
    L = _capi.lib()
    one = ctypes.c_void_p(16)

    def bad(rc, word):
        assert rc < 0 and word in L.dir_last_error(), (rc, L.dir_last_error())
    assert L.dir_crop_frames_area(None, 0, None, None, None, 0, 256, None, None, None, None) == 0          # B = 0: a no-op
    bad(L.dir_crop_frames_area(one, 16, one, None, None, 1, 256, one, None, None, None), b'null pointer')
    bad(L.dir_crop_frames_area(one, 0, one, one, None, 1, 256, one, None, None, None), b'bytes')
    bad(L.dir_crop_frames_area(one, 16, one, one, None, 1, 15, one, None, None, None), b'size')
    bad(L.dir_crop_frames_area(one, 16, one, one, None, 4097, 256, one, None, None, None), b'B 4097')
    bad(L.dir_crop_frames_area(one, 16, one, one, None, 1, 256, ctypes.c_void_p(18), None, None, None), b'aligned')
