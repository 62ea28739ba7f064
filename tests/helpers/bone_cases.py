"""Hostile joint geometry for the bone kernels (bone_proj, the factorised bone fusion and their backward passes), pure numpy.

Joints are laid out in PIXEL units x and stored the way the kernels take them, uv = 2 x / S - 1 (float32).  For S in {16, 32, 64} and
integer or half-integer x both directions of that map are exact in float32, so a joint that is meant to sit on a pixel centre, a pixel edge
or the image corner sits there bit for bit -- in the kernels and in the float32 restatement oracle.tokens.bone_proj alike.  distance = S / 16
as the engine uses; features are |N(0,1)| + 0.5 > 0, so a pixel inside a capsule never rasterises to 0 and `value != 0` IS the mask.

Samples (each [2 hands, 21 joints, 2] in pixel units; `uv_of` converts):
  ties(S)    every finger is: an axis-aligned bone from the wrist on pixel centres, a second axis-aligned bone at right angles, a 3-4-5
             diagonal, and a zero-length bone.  Axis-aligned bones on pixel centres have pixels at EXACTLY `distance` (strict comparison:
             outside); the diagonal's unit direction is not exact in float32, so its mathematical ties are decided by rounding -- the case an
             FMA contraction or a hypot that is not correctly rounded flips.  The right hand is the left one transposed, in the far corner.
  edges(S)   a joint on the image corner (uv = -1), bones across every edge and through the corners, a bone along y = -0.5 (row 0 at exactly
             distance 1), the full diagonal, a bone of 1e-4 pixels, bones along the last row / column of pixel centres, a ring of bones
             outside the image, joints at uv = +-50 and a finger that never comes near the image.
  seams(S)   horizontal bones lying ON every row y at which a workgroup's pixel strip of the fusion kernels ends (256-pixel strips in the 16-bit
             kernels, 128-pixel strips in the fp32 ones), joined by diagonal and vertical bones that cross those rows.
  poison(S)  ties(S) with NaN, +Inf and -Inf joints, in different fingers of both hands (POISON lists them).
  plain(S,n) seeded uniform joints in [-1.2, 1.2]^2.
borders(S) = [edges(S), seams(S)].
"""
import numpy as np

PARENT = [0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
CHILD = list(range(1, 21))
SIZES = (16, 32, 64)
CSEL = tuple(k * 11 for k in range(6))          # the feature channels the one-hot fusion weights select: c_n = (n % 6) * 11

# (hand, joint, (x, y)) of the poisoned joints; None = that coordinate keeps its `ties` value
POISON = ((0, 6, (np.nan, np.nan)), (0, 18, (np.inf, np.inf)), (1, 11, (-np.inf, -np.inf)), (1, 3, (np.nan, None)))


def distance(S):
    return S // 16


def uv_of(x_px, S):
    """pixel units -> the stored float32 uv (exact for integer / half-integer coordinates at S in SIZES)"""
    return (2.0 * np.asarray(x_px, np.float64) / S - 1.0).astype(np.float32)


def px_of(uv, S):
    """the kernels' own map back to pixel units, in float32 and in the reference's operation order (models/dir.py:150)"""
    uv = np.asarray(uv, np.float32)
    with np.errstate(all='ignore'):
        return ((uv + np.float32(1)) / np.float32(2) * np.float32(S)).astype(np.float32)


def _ties_left():
    j = np.zeros((21, 2))
    j[0] = (3.5, 3.5)
    j[1:5] = [(7.5, 3.5), (7.5, 7.5), (10.5, 11.5), (10.5, 11.5)]         # thumb: horizontal, vertical, 3-4-5, zero length
    j[5:9] = [(3.5, 7.5), (7.5, 7.5), (11.5, 10.5), (11.5, 10.5)]         # the thumb transposed
    j[9:13] = [(11.5, 3.5), (11.5, 1.5), (14.5, 5.5), (14.5, 5.5)]        # long horizontal, short vertical (upwards), 3-4-5
    j[13:17] = [(3.5, 12.5), (8.5, 12.5), (12.5, 15.5), (12.5, 15.5)]     # long vertical, horizontal, 4-3-5
    j[17:21] = [(1.5, 3.5), (1.5, 9.5), (5.5, 12.5), (5.5, 12.5)]         # horizontal leftwards, vertical, 4-3-5
    return j


def ties(S):
    left = _ties_left()
    right = left[:, ::-1] + (S - 16)                                     # transposed, in the bottom-right 16 x 16 pixels
    return np.stack([left, right])


def edges(S):
    far = 25.5 * S                                                       # uv = +50
    near = -24.5 * S                                                     # uv = -50
    h = S / 2
    L = np.zeros((21, 2))
    L[0] = (0, 0)                                                        # uv = -1: the image corner
    # full diagonal, across the bottom edge twice, 1e-4 px.  The two 1e-4-pixel bones sit on pixel CORNERS: at a pixel centre that is one of
    # their joints, w_a = 1 - d_a / (d_a + d_b) has d_a ~ 1e-6 (the reference's eps) and d_b ~ 1e-4, a gradient ~1e4 times any other with a
    # condition number to match -- the float32 rounding of the joint position alone would move it by 1 %
    L[1:5] = [(S, S), (S - 3.5, S + 2.5), (S - 6, S - 3), (S - 6 + 1e-4, S - 3)]
    L[5:9] = [(-2.5, 3.5), (3.5, 5.5), (4.5, -2.5), (9.5, -0.5)]         # across the left edge, the top edge, ...
    L[9:13] = [(2.5, -0.5), (10.5, -0.5), (S + 2.5, 3.5), (S - 1.5, -2.5)]   # ALONG y = -0.5, across the right edge, past the top-right corner
    L[13:17] = [(-6, -6), (-6, S + 6), (S + 6, S + 6), (S + 6, -6)]      # a ring outside the image (bone 12 leaves through the corner)
    L[17:21] = [(S - 0.5, 0.5), (S - 0.5, S - 0.5), (0.5, S - 0.5), (0.5, 0.5)]   # along the outermost pixel centres
    R = np.zeros((21, 2))
    R[0] = (far, far)                                                    # uv = +50
    R[1:5] = [(near, far), (S + 5.5, S + 7.5), (S + 9.5, S + 5.5), (S + 20.5, S + 5.5)]   # a finger that never comes near the image
    R[5:9] = [(h + 0.5, h + 0.5), (h + 0.5, S + 3.5), (-3.5, S - 2.5), (near, near)]      # in through the corner (S, S), out below, out left
    R[9:13] = [(S - 0.5, h + 0.5), (S + 0.5, h + 0.5), (S, 0), (h, 0)]   # one pixel across the right edge, to the corner joint, along y = 0
    R[13:17] = [(0, S), (0, h), (0.5, 0.5), (S - 0.5, S - 0.5)]          # corner joint, along x = 0, the diagonal through pixel centres
    R[17:21] = [(h, h), (h, h + 1e-4), (h + 4, h - 3), (0, 0)]           # 1e-4 px, 3-4-5, to the corner uv = -1
    return np.stack([L, R])


# (hand, bone) of edges(S) whose capsule cannot reach any pixel centre: their bounding boxes must be empty
EDGES_OFF_IMAGE = ((0, 13), (0, 14), (0, 15), (1, 0), (1, 1), (1, 2), (1, 3))


def seam_rows(S):
    """rows y at which a pixel strip of the fusion kernels ends inside the image: 128-pixel strips (fp32 kernels, not at S = 64) and
    256-pixel strips (16-bit kernels)"""
    rows = set()
    for strip in ((128, 256) if S <= 32 else (256,)):
        r = strip // S
        rows.update(range(r, S, r))
    return sorted(rows)


def seams(S):
    rows = seam_rows(S)
    out = np.zeros((2, 21, 2))
    for hand in range(2):
        out[hand, 0] = (S / 2 + 0.5, S / 2 - 0.5) if hand == 0 else (S / 2 - 1.5, S / 2 + 0.5)
        for f in range(5):
            s1 = rows[(hand * 10 + 2 * f) % len(rows)]
            s2 = rows[(hand * 10 + 2 * f + 1) % len(rows)]
            xa, xb = 1.5 + f, S - 2.5 - f
            out[hand, 4 * f + 1:4 * f + 5] = [(xa, s1), (xb, s1), (xb, s2), (xa, s2)]
    return out


def borders(S):
    return [edges(S), seams(S)]


def poison_uv(S):
    uv = uv_of(ties(S), S)
    for hand, j, (x, y) in POISON:
        if x is not None:
            uv[hand, j, 0] = x
        if y is not None:
            uv[hand, j, 1] = y
    return uv


def poisoned_bones():
    """[2, 20] bool: bones with a poisoned end joint"""
    m = np.zeros((2, 20), bool)
    for hand, j, _ in POISON:
        for k in range(20):
            if PARENT[k] == j or CHILD[k] == j:
                m[hand, k] = True
    return m


def plain_uv(S, n, seed=0):
    rng = np.random.default_rng(1000 * S + seed)
    return rng.uniform(-1.2, 1.2, (n, 2, 21, 2)).astype(np.float32)


def samples(S, nplain=1):
    """-> (names, uv [n, 2, 21, 2] float32): ties, edges, seams, poison, plain..."""
    names = ['ties', 'edges', 'seams', 'poison'] + ['plain%d' % i for i in range(nplain)]
    uv = [uv_of(ties(S), S), uv_of(edges(S), S), uv_of(seams(S), S), poison_uv(S)] + list(plain_uv(S, nplain))
    return names, np.stack(uv).astype(np.float32)


def features(n, seed=0):
    """[n, 42, 64] float32, |N(0,1)| + 0.5"""
    rng = np.random.default_rng(77 + seed)
    return (np.abs(rng.standard_normal((n, 42, 64))) + 0.5).astype(np.float32)


# ---------------------------------------------------------------------------------------------- closed forms (integer arithmetic)
def axis_aligned(x_px):
    """[..., 21, 2] pixel units -> [..., 20] bool: bones of non-zero length along x or y whose ends have half-integer / integer coordinates"""
    x = np.asarray(x_px, np.float64)
    a, b = x[..., PARENT, :], x[..., CHILD, :]
    grid = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    with np.errstate(all='ignore'):
        grid &= (np.abs(2 * a) < 4096).all(-1) & (np.abs(2 * b) < 4096).all(-1) & (2 * a == np.round(2 * a)).all(-1) & (2 * b == np.round(2 * b)).all(-1)
        same_x, same_y = a[..., 0] == b[..., 0], a[..., 1] == b[..., 1]
    return grid & (same_x ^ same_y)


def closed_form_axis(a, b, S, dist):
    """one axis-aligned bone a -> b (pixel units, multiples of 0.5): (inside [S(y), S(x)] bool, tie [S, S] bool) from the squared distance in
    doubled integer coordinates -- inside: d^2 < dist^2, tie: d^2 == dist^2, no rounding anywhere"""
    a2, b2 = np.round(2 * np.asarray(a)).astype(np.int64), np.round(2 * np.asarray(b)).astype(np.int64)
    c2 = 2 * np.arange(S, dtype=np.int64) + 1                             # doubled pixel centres
    px, py = np.meshgrid(c2, c2, indexing='xy')                           # [y, x]
    lo, hi = np.minimum(a2, b2), np.maximum(a2, b2)
    dx = np.maximum(np.maximum(lo[0] - px, px - hi[0]), 0)
    dy = np.maximum(np.maximum(lo[1] - py, py - hi[1]), 0)
    d2 = dx * dx + dy * dy                                                # (2 d)^2
    thr = (2 * dist) ** 2
    return d2 < thr, d2 == thr


def count_exact_ties(x_px, S, dist):
    """number of on-image pixels at EXACTLY `dist` from an axis-aligned bone of one sample [2, 21, 2]"""
    x = np.asarray(x_px, np.float64)
    ax = axis_aligned(x)
    n = 0
    for hand in range(2):
        for k in range(20):
            if ax[hand, k]:
                n += int(closed_form_axis(x[hand, PARENT[k]], x[hand, CHILD[k]], S, dist)[1].sum())
    return n
