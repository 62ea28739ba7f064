"""CPU: tests/helpers/bone_cases.py (hostile joint geometry for the bone kernels) pinned to the float32 restatement oracle.tokens.bone_proj,
which is the reference of tests/test_gpu_bone_hostile.py.  Nothing here imports the kernels.

  * pixel coordinates survive uv = 2 x / S - 1 and back exactly (all joints but the two 1e-4-pixel ones of `edges`);
  * for every axis-aligned bone on half-integer / integer coordinates the restatement's mask equals the closed-form set
    squared distance < distance^2 evaluated in integer arithmetic on doubled coordinates: pixels at exactly `distance` are outside;
  * the tie fixtures keep their point: at least 24 pixels per sample at exactly `distance` (ties and edges, every S), the 3-4-5 diagonals
    have mathematical ties that float32 rounding decides, and a bone lies on every strip seam;
  * zero-length, NaN and +-Inf bones and the off-image bones rasterise to nothing and the image stays finite;
  * oracle.spatial_grad.bone_proj_backward is finite on ties and borders."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import bone_cases as BC  # noqa: E402

from oracle import tokens as OT  # noqa: E402
from oracle.spatial_grad import bone_proj_backward  # noqa: E402


def masks(uv, S):
    """uv [n, 2, 21, 2] -> restatement mask [n, 2, S(y), S(x), 20] and image finiteness"""
    n = uv.shape[0]
    feat = BC.features(n)[:, :, :2]
    out = []
    for h in range(2):
        img, m = OT.bone_proj(uv[:, h], feat[:, 21 * h:21 * h + 21], S, BC.distance(S), return_mask=True)
        assert np.isfinite(img).all()
        assert np.array_equal((img.reshape(n, 20, 2, S, S) != 0).all(2).transpose(0, 2, 3, 1), m)        # value != 0 IS the mask
        assert np.array_equal((img.reshape(n, 20, 2, S, S) != 0).any(2).transpose(0, 2, 3, 1), m)
        out.append(m)
    return np.stack(out, 1)


@pytest.mark.parametrize('S', BC.SIZES)
def test_pixel_coordinates_come_back_exactly(S):
    for name, x in (('ties', BC.ties(S)), ('edges', BC.edges(S)), ('seams', BC.seams(S))):
        uv = BC.uv_of(x, S)
        assert uv.dtype == np.float32
        back = BC.px_of(uv, S)
        half = (2 * x == np.round(2 * x)).all(-1)                         # joints on integer / half-integer coordinates
        assert half.sum() == (40 if name == 'edges' else 42), name
        assert np.array_equal(back[half].astype(np.float64), x[half]), name
        assert np.array_equal((uv.astype(np.float64)[half] + 1) / 2 * S, x[half]), name
    e = BC.uv_of(BC.edges(S), S)
    assert (e[0, 0] == -1).all() and (e[1, 0] == 50).all() and (e[1, 8] == -50).all() and (e[1, 20] == -1).all()


@pytest.mark.parametrize('S', BC.SIZES)
def test_axis_aligned_masks_equal_the_integer_closed_form(S):
    d = BC.distance(S)
    xs = [BC.ties(S), BC.edges(S), BC.seams(S)]
    m = masks(np.stack([BC.uv_of(x, S) for x in xs]), S)
    checked = 0
    for i, x in enumerate(xs):
        ax = BC.axis_aligned(x)
        for hand in range(2):
            for k in range(20):
                if not ax[hand, k]:
                    continue
                inside, tie = BC.closed_form_axis(x[hand, BC.PARENT[k]], x[hand, BC.CHILD[k]], S, d)
                assert np.array_equal(m[i, hand, :, :, k], inside), (S, i, hand, k)
                assert not (m[i, hand, :, :, k] & tie).any()               # strict comparison: exact ties are outside
                checked += 1
    assert checked >= 40


@pytest.mark.parametrize('S', BC.SIZES)
def test_fixtures_keep_their_point(S):
    d = BC.distance(S)
    for name, x in (('ties', BC.ties(S)), ('edges', BC.edges(S))):
        n = BC.count_exact_ties(x, S, d)
        print('S=%d %s: %d pixels at exactly `distance` from an axis-aligned bone' % (S, name, n))
        assert n >= 24, (S, name, n)
    # thumb bones 0 and 1 of `ties`: 12 exact ties each at S = 16 and 32
    t = BC.ties(S)
    if S <= 32:
        for k in (0, 1):
            assert BC.closed_form_axis(t[0, BC.PARENT[k]], t[0, BC.CHILD[k]], S, d)[1].sum() == 12
    # the 3-4-5 diagonals (bone 4 f + 2 of every finger): pixels whose float64 distance equals `distance` to 1e-12 are mathematical ties
    # (all coordinates are multiples of 0.1 there); the float32 restatement decides them by rounding
    uv = BC.uv_of(t, S)[None]
    m = masks(uv, S)[0]
    c = np.arange(S) + 0.5
    px, py = np.meshgrid(c, c, indexing='xy')
    ties_math = kept = 0
    for hand in range(2):
        for k in range(2, 20, 4):
            a, b = t[hand, BC.PARENT[k]], t[hand, BC.CHILD[k]]
            assert np.hypot(*(b - a)) == 5.0
            u = (b - a) / 5.0
            s = np.clip((px - a[0]) * u[0] + (py - a[1]) * u[1], 0, 5)
            dist = np.hypot(px - a[0] - s * u[0], py - a[1] - s * u[1])
            tie = np.abs(dist - d) < 1e-12
            ties_math += int(tie.sum())
            kept += int((m[hand, :, :, k] & tie).sum())
            assert np.array_equal(m[hand, :, :, k] & ~tie, (dist < d) & ~tie), (S, hand, k)      # away from the ties float32 and float64 agree
    print('S=%d ties: %d mathematical ties on the 3-4-5 diagonals, the float32 restatement keeps %d' % (S, ties_math, kept))
    assert ties_math >= 6
    if S == 16:
        assert 0 < kept < ties_math                                      # rounding decides: some in, some out
    # seams: a horizontal bone lies on every row at which a pixel strip ends
    sm = BC.seams(S)
    rows = set()
    for hand in range(2):
        for k in range(20):
            a, b = sm[hand, BC.PARENT[k]], sm[hand, BC.CHILD[k]]
            if a[1] == b[1] and a[0] != b[0]:
                rows.add(int(a[1]))
    assert set(BC.seam_rows(S)) <= rows, (BC.seam_rows(S), rows)
    if S == 32:
        assert BC.seam_rows(S) == [4, 8, 12, 16, 20, 24, 28]


@pytest.mark.parametrize('S', BC.SIZES)
def test_degenerate_and_poisoned_bones_rasterise_to_nothing(S):
    names, uv = BC.samples(S, 1)
    m = masks(uv, S)                                                      # asserts a finite image, too
    i_t, i_e, i_p = names.index('ties'), names.index('edges'), names.index('poison')
    for hand in range(2):
        for k in range(3, 20, 4):                                         # zero length
            assert not m[i_t, hand, :, :, k].any()
    for hand, k in BC.EDGES_OFF_IMAGE:
        assert not m[i_e, hand, :, :, k].any(), (hand, k)
    pb = BC.poisoned_bones()
    assert pb.sum() == 8 and pb[0].any() and pb[1].any()
    for hand in range(2):
        for k in range(20):
            if pb[hand, k]:
                assert not m[i_p, hand, :, :, k].any(), (hand, k)
            else:
                assert np.array_equal(m[i_p, hand, :, :, k], m[i_t, hand, :, :, k])
    assert not np.isfinite(uv[i_p]).all() and np.isnan(uv[i_p]).any() and np.isposinf(uv[i_p]).any() and np.isneginf(uv[i_p]).any()
    # every other bone of ties / edges / seams touches the image somewhere, except the listed ones
    assert m[i_t].any((1, 2)).sum() == 2 * 15


@pytest.mark.parametrize('S', [16, 32])
def test_reference_gradient_is_finite_on_ties_and_borders(S):
    xs = [BC.ties(S)] + BC.borders(S)
    uv = np.stack([BC.uv_of(x, S) for x in xs])
    n = len(xs)
    feat = BC.features(n)
    rng = np.random.default_rng(5)
    for hand in range(2):
        g_img = rng.standard_normal((n, 1280, S, S)).astype(np.float32)
        g_uv, g_feat = bone_proj_backward(uv[:, hand], feat[:, 21 * hand:21 * hand + 21], g_img, S, BC.distance(S))
        assert np.isfinite(g_uv).all() and np.isfinite(g_feat).all()
        for f in range(5):                                                # ties: the tip of a zero-length bone receives nothing
            assert (g_uv[0, 4 * f + 4] == 0).all() and (g_feat[0, 4 * f + 4] == 0).all()
