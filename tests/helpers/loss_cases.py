"""TEST INFRASTRUCTURE (CPU only: numpy + torch CPU): the per-element gate of the loss kernels of csrc/loss.hip -- dir_stage_losses_forward /
_backward (stage_loss_kernel, stage_reduce_kernel, stage_loss_bwd_kernel) and dir_dense_losses_forward / _backward (dense_pixel_kernel,
radix_hist_kernel, radix_scatter_kernel, lovasz_kernel, dense_final_kernel and their backward twins).

GATE   every output element: |got - ref64| <= c 2^-24 S + widen + floor, floor = half an ulp of a float32 output + 2^-149.  ref64 = the float64 evaluation of the same formula on the float32
operands (the constants 0.15f, 0.01f, 0.005f, 1e-12f and the backward's 0.1f are float32 numbers too), S the element's first-order error
scale, c one constant per output kind (CONSTANTS below), widen = 0 off the undecided band.

RESTATEMENT   The reference's modules -- models/dir.py:542-594 (the loss block), models/loss.py:11-33 (NormalVectorLoss), :41-60
(EdgeLengthLoss), :68-85 (SmoothL1Loss, knee 0.01), models/lovasz_loss.py:19-31,155-202 (lovasz_softmax on the raw logits) -- are restated
once, stage_eval() / dense_eval(), over an arithmetic `A`: A64 carries V = (float64 value, running error bound e of the float32 evaluation),
A32 is numpy float32 in the order loss.hip documents (elementwise float32 without contraction, corner sums in the kernel's add order, vertex
sums in CSR order, float64 for the term sums, the cross entropy's exp / log / softmax and the Jaccard scan, as the kernels have them).  torch_stage() / torch_dense() restate the modules in torch for CPU
float32 autograd.  The dense side builds on oracle/losses.py (interpolation taps, stable argsort).

ERROR SCALE, STAGE   u = 2^-24, S = e / u, e carried per operation like tests/helpers/mano_cases.py:
    float32 inputs            e = 0                              c = a +- b   e = e(a) + e(b) + u |c|
    c = a b                   |b| e(a) + |a| e(b) + u |c|        c = a / b    e(a) / |b| + |a| e(b) / b^2 + u |c|
    c = sqrt(a)               e(a) / sqrt(max(a, e(a))) + u |c|  max(a, k), |a|, a sign: e passes through
  SmoothL1 element  z = x - y, x = p / 0.15, y = (gt - center) / 0.15: e(z) = u (|x| + 2 |y| + |z|) -- the subtraction gt - center of two float32
  numbers costs u |gt - center|, NOT u |center| (the cancellation at coordinates of 1e3 loses nothing the inputs had), so this is tighter than
  |d term / dz| (|x| + |y| + |c|) + |term|; the term: |term'(z)| e(z) + 3 u |term| (+ the product's u).  Edge: the same through d = p_a - p_b, sumsq,
  + 1e-12, sqrt, |len - leng|.  Normal: through the three normalisations (e / max(|v|, 1e-12): S grows like 1 / |edge|), the cross product and
  the dot.  Term sums are float64 in the kernel: S of scratch[b][k] is the MEAN of its elements' scales; out13[k] adds u |out|.
  Backward: every contribution (edge: sgn(len - leng) d / len ke; normal: sgn(v.n) (n - (v.n) v) / |e| kn) carries its own e; a vertex sums its
  corners (CSR lists) with e = sum e_i + n u sum |contribution_i|, plus the SmoothL1 part km term'(z), then / 0.15 and u |g|.
UNDECIDED BAND (stage backward)   sgn(len - leng) and sgn(v.n): where |argument| <= BAND e(argument) the reference takes 0 for that one
contribution and the vertex's bound is widened by the contribution's magnitude (either sign passes); BAND = 1: the argument within its own bound.  Cap:
1 % of a case's gradient elements (the degenerate class apart).

DENSE   The Lovasz permutation is exact: errors fl32(|fg - logit|), descending, stable in p = b S S + pix = np.argsort(-err32, kind='stable').
sign(logit - fg) is exact, so grad_seg has no band: S = |gce| + |glov| + |g| WRITTEN WITH ABSOLUTE VALUES, |gce| = kce (softmax_c + [c == y]) and
|glov| = klv (|J_i| + |q_i| + |J_{i-1}| + |q_{i-1}|), J = 1 - q: a float32 evaluation forms softmax - 1 and J_i - J_{i-1} by cancellation, so with the plain magnitudes the
float32 references sit 7e6 units out and c would accept anything; this S is smaller than that c S on every element.  grad_dense inside the knee (|z| <= 0.0101) reveals the bilinear
target: S = kd (|x| + T) + |g|, T = 3 sum_taps |w| |gt| + the weights' own error 3 (src + 1) (|gt_a| + |gt_b|) per axis (a weight is src - floor(src), src
up to 256, and another valid float32 order of (dst + 0.5) in / out - 0.5 moves it by u src: torch's does); outside S = |g|.  Scalars: seg and lovasz are float64 sums of float64 terms rounded once
(S = |out|); dense: the mean of |term'| (T + |z|) + 3 |term|, times dense_weight, + |out|.  The interpolation weights are float32
numbers computed in torch's order (oracle/losses.py: interpolate_bilinear) and are operands.

CONSTANTS   c(kind) = 4 x the largest |ref32 - ref64| / (u S) over the list, off the band; ref32 = the worse of (a) torch CPU float32 autograd
through the restatement, one thread, and (b) A32.  Not measured on the kernels.  RATIOS records (a) and (b); tests/test_loss_cases_ref.py
re-measures them.  (grad_seg: (a) forms J_i - J_{i-1} in float32, a cancellation of ~1 / dJ units that the kernel's float64 scan does not
have: it is what sets that constant.)
GRAD_SEG, SECOND GATE   With that constant the tolerance of grad_seg is ~1e-5 klv, more than whole elements at P >= 8192: a scatter that reverses ties
would pass.  loss.hip documents a float64 scan, so the kernel is ALSO held to kind 'grad_seg_scan': the same reference with the plain |glov| in S
(S = kce (softmax_c + [c == y]) + |glov| + |g|) and c = 4 x the numpy reference (b) alone, which scans in float64 as the kernel does; torch's float32
scan is not asked to meet it (FLOAT64_SCAN_ONLY).  It rejects reversed ties on every case they move.

DEGENERATE   predicted / ground-truth zero-length edges, collinear ground-truth triangles, a face that repeats an index: the reference is
undefined there (normalize(0), sign(0) under autograd).  Such cases are held to finite outputs, the gate on every element OFF the band, guards,
bit-equal repeats and the promised zeros (a predicted mesh collapsed to one point: normal term exactly 0, mesh gradient = its SmoothL1 part bit for
bit); at most 10 % of a list.

EDGES -> CASES   (dense (B, S) -> P)
    256  pixel chunk / radix chunk      (1,15) 225 | (1,16) 256 | (1,17) 289; S S % 256 != 0: S = 1, 15, 17, 46, 90, 91, 4
    2048 RS_TILE                        (7,17) 2023 | (2,32) 2048 | (129,4) 2064, (1,46) 2116
    8192 LV_T LV_E (carry, prevJ)       (1,90) 8100 | (8,32) 8192 | (1,91) 8281
    16384 second pass                   (16,32) 16384 | (2,91) 16562, (65,16) 16640
    B > 64 lane stride                  (65,16), (129,4) dense; stage B = 64 | 65, 129
    n_faces 256 (LT stride)             255 | 256 | 257; 1; 1538; 3748 = the LDS check's largest (3749 raises)
    c2 stride 2 | 3 | 5; H, W: = S, 256, 100, 37, 8 < S, 1, 96 x 64, 37 x 100 (clamps at 0 and H - 1)
"""
import collections
import functools
import zlib

import numpy as np
import torch

from dir_amd import synth
from oracle import losses as OL

U = 2.0 ** -24
TINY = 2.0 ** -149
BAND = 1.0
F32 = np.float32
NV, NJ = 778, 21
SIDES = ('left', 'right')
F_MAX = (150 * 1024 // 4 - 2 * NV * 3) // 9          # 3748: dir_stage_losses_backward's LDS check


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


# ===================================================================================================================== arithmetic
class V(object):
    """float64 value v with the running bound e of its float32 evaluation"""
    __slots__ = ('v', 'e')
    __array_ufunc__ = None

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(a):
        return a if isinstance(a, V) else V(a)

    def __add__(a, b):
        b = V.of(b); v = a.v + b.v
        return V(v, a.e + b.e + U * np.abs(v))
    __radd__ = __add__

    def __sub__(a, b):
        b = V.of(b); v = a.v - b.v
        return V(v, a.e + b.e + U * np.abs(v))

    def __rsub__(a, b):
        return V.of(b) - a

    def __neg__(a):
        return V(-a.v, a.e)

    def __mul__(a, b):
        b = V.of(b); v = a.v * b.v
        return V(v, a.e * np.abs(b.v) + np.abs(a.v) * b.e + U * np.abs(v))
    __rmul__ = __mul__

    def __truediv__(a, b):
        b = V.of(b); v = a.v / b.v
        return V(v, a.e / np.abs(b.v) + np.abs(a.v) * b.e / (b.v * b.v) + U * np.abs(v))

    def __rtruediv__(a, b):
        return V.of(b) / a

    def __getitem__(a, i):
        return V(a.v[i], a.e[i])


class A64(object):
    """float64 values with running bounds"""
    exact = True

    @staticmethod
    def lift(x):
        return V(np.asarray(x, np.float64))

    @staticmethod
    def k(x):
        return float(F32(x))

    @staticmethod
    def sqrt(a):
        r = np.sqrt(a.v)
        return V(r, a.e / np.sqrt(np.maximum(np.maximum(a.v, a.e), 1e-300)) + U * r)

    @staticmethod
    def abs(a):
        return V(np.abs(a.v), a.e)

    @staticmethod
    def maxk(a, k):
        return V(np.maximum(a.v, k), a.e)

    @staticmethod
    def where(m, a, b):
        a, b = V.of(a), V.of(b)
        return V(np.where(m, a.v, b.v), np.where(m, a.e, b.e))

    @staticmethod
    def val(a):
        return a.v

    @staticmethod
    def mean64(a, axis):
        return V(a.v.mean(axis=axis), a.e.mean(axis=axis))

    @staticmethod
    def round32(a):
        return V(a.v, a.e + U * np.abs(a.v))


class A32(object):
    """numpy float32, elementwise, no contraction"""
    exact = False

    @staticmethod
    def lift(x):
        return np.asarray(x, F32)

    @staticmethod
    def k(x):
        return F32(x)

    sqrt = staticmethod(np.sqrt)
    abs = staticmethod(np.abs)

    @staticmethod
    def maxk(a, k):
        return np.maximum(a, F32(k))

    @staticmethod
    def where(m, a, b):
        return np.where(m, a, b).astype(F32)

    @staticmethod
    def val(a):
        return a

    @staticmethod
    def mean64(a, axis):
        return a.astype(np.float64).mean(axis=axis)

    @staticmethod
    def round32(a):
        return np.asarray(a).astype(F32)


def _c3(a):
    return a[..., 0], a[..., 1], a[..., 2]


def _sumsq(a):
    x, y, z = _c3(a)
    return x * x + y * y + z * z


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _stack(A, xs):
    if A.exact:
        return V(np.stack([x.v for x in xs], -1), np.stack([x.e for x in xs], -1))
    return np.stack(xs, -1).astype(F32)


def _ex(A, s):
    """a [...] quantity as [..., 1]"""
    return V(s.v[..., None], s.e[..., None]) if A.exact else s[..., None]


def _normalize(A, a):
    n = A.maxk(A.sqrt(_sumsq(a)), A.k(1e-12))
    return a / _ex(A, n), n


def _cross(A, a, b):
    ax, ay, az = _c3(a); bx, by, bz = _c3(b)
    return _stack(A, [ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx])


def _sl1(A, x, y):
    """models/loss.py:74-81 for one element: (term, d term / dx)"""
    z = x - y
    az = A.abs(z)
    small = A.val(az) < A.k(0.01)
    term = A.where(small, A.k(0.5) * (z * z), A.k(0.01) * (az - A.k(0.005)))
    sg = np.sign(A.val(z))
    d = A.where(small, z, A.k(0.01) * (V(sg) if A.exact else sg.astype(F32)))
    return term, d


# ===================================================================================================================== stage: cases
StageCase = collections.namedtuple('StageCase', 'name B c2 proj coord_weight gout table geo degenerate')
GOUT13 = (1.0, 0.5, 0.0, 2.0, 1.25, 0.75, 3.0, 0.0, 1.5, 0.625, 0.25, 2.5, 0.875)       # 13 distinct but for the two zeros (slots 2 and 7)


@functools.lru_cache(maxsize=None)
def stage_cases():
    g, n = GOUT13, None
    L = [
        StageCase('b1_c2', 1, 2, False, 10.0, n, 'f1538', ('knee', 'same'), False),
        StageCase('b1_c5_proj_gout', 1, 5, True, 3.5, g, 'f1538', ('tiny', 'big'), False),
        StageCase('b2_c3', 2, 3, False, 10.0, g, 'f1538', ('same', 'big'), False),
        StageCase('b2_c2_proj', 2, 2, True, 10.0, n, 'f257', ('knee',), False),
        StageCase('b3_c5', 3, 5, False, 3.5, n, 'f1538', ('tiny', 'knee', 'same'), False),
        StageCase('b3_c3_proj', 3, 3, True, 10.0, g, 'f255', ('big',), False),
        StageCase('b64_c3', 64, 3, False, 10.0, g, 'f1538', ('same', 'big', 'knee', 'tiny'), False),
        StageCase('b65_c2', 65, 2, True, 3.5, g, 'f256', ('knee', 'big'), False),
        StageCase('b65_c5', 65, 5, False, 10.0, n, 'f1538', ('tiny', 'same'), False),
        StageCase('b129_c5', 129, 5, False, 3.5, g, 'f257', ('same', 'big', 'knee', 'tiny'), False),
        StageCase('b129_c3_proj', 129, 3, True, 10.0, n, 'f1', ('big',), False),
        StageCase('f1', 2, 3, False, 10.0, g, 'f1', ('same',), False),
        StageCase('f1_tiny', 2, 2, False, 10.0, n, 'f1', ('tiny',), False),
        StageCase('f255', 3, 2, False, 10.0, n, 'f255', ('tiny',), False),
        StageCase('f256', 2, 5, False, 3.5, g, 'f256', ('knee',), False),
        StageCase('f257', 1, 3, False, 10.0, g, 'f257', ('same',), False),
        StageCase('fmax', 2, 3, False, 10.0, g, 'f%d' % F_MAX, ('same', 'tiny'), False),
        StageCase('novert', 2, 3, False, 10.0, n, 'novert', ('knee',), False),
        StageCase('star300', 3, 2, False, 3.5, g, 'star300', ('big', 'same'), False),
        StageCase('zero_edges', 64, 3, False, 10.0, g, 'f1538', ('pzero', 'gzero', 'collinear', 'point'), True),
        StageCase('repeat_face', 2, 3, False, 10.0, n, 'repeat', ('same',), True),
    ]
    assert len({c.name for c in L}) == len(L)
    return tuple(L)


@functools.lru_cache(maxsize=None)
def face_tables(kind):
    """(left, right) int32 [F, 3] tables, every index in [0, 778)"""
    out = []
    for side in SIDES:
        base = np.asarray(synth.loss_faces(side), np.int64)
        rng = _rng('faces.%s.%s' % (kind, side))
        if kind.startswith('f'):
            F = int(kind[1:])
            f = base[:F]
            while f.shape[0] < F:                                            # more triangles than the synthetic table has: random, three distinct indices
                extra = np.stack([rng.permutation(NV)[:3] for _ in range(F - f.shape[0])])
                f = np.concatenate([f, extra])
        elif kind == 'novert':                                               # vertices 700..777 in no face
            f = base.copy()
            f[f >= 700] -= 100
            bad = (f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])
            f = f[~bad]
        elif kind == 'star300':                                              # vertex 5 in 300 faces (on top of its own), at every corner
            f = base.copy()
            for i in range(300):
                if 5 not in f[2 * i]:
                    f[2 * i, i % 3] = 5
        elif kind == 'repeat':                                               # face 0 repeats an index: (a, a, b)
            f = base.copy()
            f[0, 1] = f[0, 0]
        else:
            raise KeyError(kind)
        assert f.min() >= 0 and f.max() < NV and f.shape[0] <= F_MAX
        out.append(np.ascontiguousarray(f, np.int32))
    assert out[0].shape == out[1].shape
    return tuple(out)


def csr(face):
    """vertex -> (face * 3 + corner) lists, the order dir_stage_losses_backward sums in (dir_amd/models/loss.py: vertex_face_csr)"""
    flat = np.asarray(face, np.int64).reshape(-1)
    order = np.argsort(flat, kind='stable')
    off = np.zeros(NV + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(flat, minlength=NV))
    return off.astype(np.int32), order.astype(np.int32)


def geo_sample(case, geo):
    """the sample that carries hostile geometry `geo`: the last one first (tails), then spread"""
    i = case.geo.index(geo)
    return (i * 37 + case.B - 1) % case.B if i else case.B - 1


@functools.lru_cache(maxsize=None)
def stage_inputs(case):
    """float32 predictions / targets at the scales of tests/test_gpu_loss.py:_random_stage, hostile geometry on the vertices of face 0 (and 1)
    of a few samples; returns (pred, gt, faces).  pred always holds pd_mesh_uv_* (the backward's leaf); with case.proj also pd_proj_* and
    pd_mesh_uv_* = the float32 projection, which the forward recomputes from pd_proj_*."""
    rng, B, c2 = _rng('stage.' + case.name), case.B, case.c2
    faces = face_tables(case.table)
    pred, gt = {}, {}
    for side in SIDES:
        gt['center_' + side] = rng.normal(0, 0.05, (B, 1, 3)).astype(F32)
        for n, tag in ((NJ, 'joint'), (NV, 'mesh')):
            xyz = rng.normal(0, 0.05, (B, n, 3)).astype(F32)
            pred['pd_%s_xyz_%s' % (tag, side)] = xyz
            noise = np.where(rng.rand(B, n, 3) < 0.5, rng.normal(0, 0.0005, (B, n, 3)), rng.normal(0, 0.01, (B, n, 3)))
            gt['%s_3d_%s' % (tag, side)] = (xyz + gt['center_' + side] + noise).astype(F32)
            uv = rng.uniform(-1, 1, (B, n, 2)).astype(F32)
            pred['pd_%s_uv_%s' % (tag, side)] = uv
            noise = np.where(rng.rand(B, n, 2) < 0.5, rng.normal(0, 0.004, (B, n, 2)), rng.normal(0, 0.05, (B, n, 2)))
            gt['%s_2d_%s' % (tag, side)] = np.concatenate([uv + noise, rng.normal(0, 1, (B, n, c2 - 2))], axis=2).astype(F32)
    pred['pd_offset'] = rng.normal(0, 0.3, (B, 3)).astype(F32)
    for i, geo in enumerate(case.geo):
        s = geo_sample(case, geo)
        for side, face in zip(SIDES, faces):
            pm, gm, cen = pred['pd_mesh_xyz_' + side], gt['mesh_3d_' + side], gt['center_' + side]
            f0 = face[min(i, face.shape[0] - 1)]
            if geo == 'same':                                                # pred == gt exactly (centre 0): joints, uv, and the vertices of one face
                cen[s] = 0
                gm[s, f0] = pm[s, f0]
                gt['joint_3d_' + side][s] = pred['pd_joint_xyz_' + side][s]
                gt['joint_2d_' + side][s, :, :2] = pred['pd_joint_uv_' + side][s]
            elif geo == 'knee':                                              # residuals exactly representable, both sides of the knee and ON it
                k = np.array([2.0 ** -7, -2.0 ** -7, 2.0 ** -6, -2.0 ** -6, F32(0.01), -F32(0.01), 0.0, 2.0 ** -30], F32)
                g2 = gt['joint_2d_' + side]
                g2[s, :, :2] = (np.arange(NJ * 2).reshape(NJ, 2) % 5 - 2) * F32(0.25)
                pred['pd_joint_uv_' + side][s] = g2[s, :, :2] + k[np.arange(NJ * 2) % 8].reshape(NJ, 2)
                g2 = gt['mesh_2d_' + side]
                g2[s, :64, :2] = 0
                pred['pd_mesh_uv_' + side][s, :64] = k[np.arange(128) % 8].reshape(64, 2)
            elif geo == 'tiny':                                              # predicted (at the origin, where float32 resolves it) and ground-truth edges of 1e-7 in normalised units
                pm[s, f0[0]] = 0
                pm[s, f0[1]] = F32([1.5e-8, 0, 0])
                gm[s, f0[2]] = gm[s, f0[0]] + F32(1.5e-8)
            elif geo == 'big':                                               # coordinates of 1e3 against centres of 1e3
                cen[s] = (1e3 + rng.normal(0, 0.05, (1, 3))).astype(F32)
                gm[s] = (pm[s] + cen[s] + rng.normal(0, 0.002, (NV, 3))).astype(F32)
                gt['joint_3d_' + side][s] = (pred['pd_joint_xyz_' + side][s] + cen[s]).astype(F32)
            elif geo == 'point':                                             # the whole predicted mesh in one point: every triangle contribution is exactly 0
                pm[s] = pm[s, 0]
            elif geo == 'pzero':
                pm[s, f0[1]] = pm[s, f0[0]]
            elif geo == 'gzero':
                gm[s, f0[1]] = gm[s, f0[0]]
            elif geo == 'collinear':
                cen[s] = 0
                gm[s, f0[0]], gm[s, f0[1]], gm[s, f0[2]] = F32([0.0375, 0, 0]), F32([0.075, 0, 0]), F32([0.15, 0, 0])
            else:
                raise KeyError(geo)
    if case.proj:
        for side in SIDES:
            proj = np.concatenate([rng.uniform(2, 6, (B, 1)), rng.normal(0, 0.2, (B, 2))], axis=1).astype(F32)
            pred['pd_proj_' + side] = proj
            uv = (proj[:, None, :1] * pred['pd_mesh_xyz_' + side][..., :2]).astype(F32) + proj[:, None, 1:]
            pred['pd_mesh_uv_' + side] = uv.astype(F32)
            gt['mesh_2d_' + side][..., :2] = (uv + rng.normal(0, 0.01, (B, NV, 2))).astype(F32)
    for d in (pred, gt):
        for k in d:
            d[k] = np.ascontiguousarray(d[k], F32)
            d[k].setflags(write=False)
    return pred, gt, faces


STAGE_GRADS = tuple('pd_%s_%s' % (t, s) for t in ('joint_uv', 'mesh_uv', 'joint_xyz', 'mesh_xyz') for s in SIDES) + ('pd_offset',)
STAGE_TERM_KIND = ('sl1',) * 8 + ('edge',) * 2 + ('normal',) * 2 + ('sl1',)


def stage_kind(name, k=None):
    """the constant's key of an output (k: term slot of scratch / out13)"""
    if name in ('scratch', 'out13'):
        return '%s_%s' % (name, STAGE_TERM_KIND[k])
    return 'g_' + name[3:].rsplit('_', 1)[0] if name != 'pd_offset' else 'g_offset'


# ===================================================================================================================== stage: restatement
def _scatter(A, corners, face, skip_last):
    """vertex sums of the [B, 3F, 3] corner contributions in CSR order; V: also the bound of the sequential float32 sum"""
    off, order = csr(face)
    order = order.astype(np.int64)
    vert = np.asarray(face, np.int64).reshape(-1)[order]
    if skip_last:
        last = np.zeros(order.shape[0], bool)
        last[off[1:][off[1:] > off[:-1]] - 1] = True
        order, vert = order[~last], vert[~last]
    B = A.val(corners).shape[0]
    if A.exact:
        v, e, a = (np.zeros((B, NV, 3)) for _ in range(3))
        np.add.at(v, (slice(None), vert), corners.v[:, order])
        np.add.at(e, (slice(None), vert), corners.e[:, order])
        np.add.at(a, (slice(None), vert), np.abs(corners.v[:, order]))
        n = np.bincount(vert, minlength=NV).astype(np.float64)[None, :, None]
        return V(v, e + U * n * a)
    g = np.zeros((B, NV, 3), F32)
    np.add.at(g, (slice(None), vert), corners[:, order])
    return g


def stage_eval(A, case, defect=None):
    """Every output of dir_stage_losses_forward / _backward for `case` in arithmetic A.  Returns {name: values}; with A64 the values are V and
    'widen:<name>' / 'band:<name>' hold the undecided band of pd_mesh_xyz_*."""
    pred, gt, faces = stage_inputs(case)
    B, c2 = case.B, case.c2
    gout = np.ones(13, F32) if case.gout is None else np.asarray(case.gout, F32)
    gk = lambda k, h=0: A.k(gout[k + (1 - h if defect == 'left_right_swapped' and k < 12 else h)])  # noqa: E731
    cw, invB = A.k(case.coord_weight), A.k(F32(1.0) / F32(B))
    k015 = A.k(0.15)
    scratch, out = [None] * 13, {}
    for h, (side, face) in enumerate(zip(SIDES, faces)):
        F = face.shape[0]
        cen = A.lift(gt['center_' + side])
        pm = A.lift(pred['pd_mesh_xyz_' + side]) / k015
        gm = (A.lift(gt['mesh_3d_' + side]) - cen) / k015
        pj = A.lift(pred['pd_joint_xyz_' + side]) / k015
        gj = (A.lift(gt['joint_3d_' + side]) - cen) / k015

        def target2d(name, n):
            t = gt[name + side]
            if defect == 'c2_stride_2':                                      # ((b n + j) 2 + c) into the flat [B, n, c2] array
                idx = (np.arange(B * n)[:, None] * 2 + np.arange(2)[None, :]).reshape(B, n, 2)
                return A.lift(t.reshape(-1)[idx])
            return A.lift(t[:, :, :2])
        # ---- SmoothL1 terms and gradients (models/dir.py:572-577; models/loss.py:68-85)
        t, d = _sl1(A, A.lift(pred['pd_joint_uv_' + side]), target2d('joint_2d_', NJ))
        scratch[0 + h] = A.mean64(t, (1, 2))
        out['pd_joint_uv_' + side] = gk(0, h) * cw * invB / A.k(NJ * 2.0) * d
        muv = A.lift(pred['pd_mesh_uv_' + side])
        if case.proj:                                                        # utils/utils.py:47-63 inside the forward kernel
            pr = A.lift(pred['pd_proj_' + side])
            fwd = pr[:, None, :1] * A.lift(pred['pd_mesh_xyz_' + side])[:, :, :2] + pr[:, None, 1:]
        else:
            fwd = muv
        m2d = target2d('mesh_2d_', NV)
        scratch[2 + h] = A.mean64(_sl1(A, fwd, m2d)[0], (1, 2))
        out['pd_mesh_uv_' + side] = gk(2, h) * cw * invB / A.k(NV * 2.0) * _sl1(A, muv, m2d)[1]
        t, d = _sl1(A, pj, gj)
        scratch[4 + h] = A.mean64(t, (1, 2))
        out['pd_joint_xyz_' + side] = gk(4, h) * cw * invB / A.k(NJ * 3.0) * d / k015
        t, dm = _sl1(A, pm, gm)
        scratch[6 + h] = A.mean64(t, (1, 2))
        # ---- triangles (models/loss.py:46-60 and :16-33)
        P = [pm[:, face[:, c]] for c in range(3)]
        G = [gm[:, face[:, c]] for c in range(3)]
        nsrc = P if defect == 'normal_from_prediction' else G
        ng, _ = _normalize(A, _cross(A, _normalize(A, nsrc[1] - nsrc[0])[0], _normalize(A, nsrc[2] - nsrc[0])[0]))
        se, sn = (10, 8) if defect == 'edge_normal_swapped' else (8, 10)
        ke = gk(se, h) * invB / A.k(F32(3.0) * F32(F))
        kn = gk(sn, h) * A.k(0.1) * invB / A.k(F32(3.0) * F32(F))
        acc = [[], [], []]                                                   # per corner: its contributions in the kernel's add order
        wid = [np.zeros((B, F, 3)) for _ in range(3)]
        e_terms, n_terms = [], []
        for ea, eb in ((0, 1), (0, 2), (1, 2)):
            dd = P[ea] - P[eb]
            if defect == 'eps_outside_sqrt':
                ln_e, ln_g = A.sqrt(_sumsq(dd)) + A.k(1e-12), A.sqrt(_sumsq(G[ea] - G[eb])) + A.k(1e-12)
            else:
                ln_e, ln_g = A.sqrt(_sumsq(dd) + A.k(1e-12)), A.sqrt(_sumsq(G[ea] - G[eb]) + A.k(1e-12))
            diff = ln_e - ln_g
            e_terms.append(A.abs(diff))
            ev = P[eb] - P[ea]
            v, ln = _normalize(A, ev)
            dt = _dot(v, ng)
            n_terms.append(A.abs(dt))
            tt = ng - _ex(A, dt) * v
            if A.exact:
                for arg, mag, hi, lo in ((diff, dd / _ex(A, ln_e) * ke, ea, eb), (dt, tt / _ex(A, ln) * kn, eb, ea)):
                    band = np.abs(arg.v) <= BAND * arg.e
                    sg = np.where(band, 0.0, np.sign(arg.v))[..., None]
                    c = V(sg * mag.v, np.where(band[..., None], 0.0, mag.e))
                    w = np.where(band[..., None], np.abs(mag.v) + mag.e, 0.0)
                    acc[hi].append(c); acc[lo].append(-c)
                    wid[hi] += w; wid[lo] += w
            else:
                s = (np.sign(diff) / ln_e * ke).astype(F32)[..., None]
                acc[ea].append(s * dd); acc[eb].append(-s * dd)
                sc = (np.sign(dt) / ln * kn).astype(F32)[..., None]
                acc[eb].append(sc * tt); acc[ea].append(-(sc * tt))
        scratch[8 + h] = A.mean64(_stack(A, e_terms), (1, 2))
        scratch[10 + h] = A.mean64(_stack(A, n_terms), (1, 2))
        corners = []
        for c in range(3):
            s = acc[c][0]
            for x in acc[c][1:]:
                s = s + x
            corners.append(s)
        if A.exact:
            corners = V(np.stack([x.v for x in corners], 2).reshape(B, F * 3, 3), np.stack([x.e for x in corners], 2).reshape(B, F * 3, 3))
        else:
            corners = np.stack(corners, 2).reshape(B, F * 3, 3)
        skip = defect == 'last_csr_corner_skipped'
        vs = _scatter(A, corners, face, skip)
        km = gk(6, h) * cw * invB / A.k(NV * 3.0)
        out['pd_mesh_xyz_' + side] = (vs + km * dm) / k015
        if A.exact:
            w = np.zeros((B, NV, 3))
            np.add.at(w, (slice(None), np.asarray(face, np.int64).reshape(-1)), np.stack(wid, 2).reshape(B, F * 3, 3))
            out['widen:pd_mesh_xyz_' + side] = w / float(F32(0.15))
            out['band:pd_mesh_xyz_' + side] = w > 0
    # ---- offset (models/dir.py:561,591-592)
    y = (A.lift(gt['center_right']) - A.lift(gt['center_left']))[:, 0] / k015
    t, d = _sl1(A, A.lift(pred['pd_offset']), y)
    scratch[12] = A.mean64(t, 1)
    out['pd_offset'] = gk(12) * cw * (A.k(1.0) if defect == 'offset_without_1_over_B' else invB) / A.k(3.0) * d
    if A.exact:
        sc = V(np.stack([s.v for s in scratch], 1), np.stack([s.e for s in scratch], 1))
        w = np.array([float(F32(case.coord_weight)) if (k < 8 or k == 12) else (1.0 if k < 10 else 0.1) for k in range(13)])
        m = V(sc.v.mean(0) * w, sc.e.mean(0) * w)
        out['scratch'], out['out13'] = sc, A.round32(m)
        for k in STAGE_GRADS:                                                # the kernel's final store is one more rounding only where a division follows; u |g| covers it
            out[k] = V(out[k].v, out[k].e + U * np.abs(out[k].v))
    else:
        sc = np.stack(scratch, 1)
        w = np.array([float(F32(case.coord_weight)) if (k < 8 or k == 12) else (1.0 if k < 10 else 0.1) for k in range(13)])
        out['scratch'], out['out13'] = sc, (sc.mean(0) * w).astype(F32)
        for k in STAGE_GRADS:
            out[k] = np.asarray(out[k], F32)
    return out


def torch_stage(case):
    """(a): torch CPU float32 autograd through the loss modules (models/loss.py) as models/dir.py:571-592 calls them"""
    pred, gt, faces = stage_inputs(case)
    T = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    leaves = {k: T(pred[k]).requires_grad_(True) for k in STAGE_GRADS}
    gout = torch.ones(13) if case.gout is None else torch.tensor(case.gout, dtype=torch.float32)

    def sl1(x, y):                                                           # per sample mean of the two branches, then the batch mean
        z = x.reshape(x.shape[0], -1) - y.reshape(x.shape[0], -1)
        az = z.abs()
        small = az < 0.01
        per = torch.where(small, 0.5 * z * z, torch.zeros_like(z)).mean(1) + torch.where(~small, 0.01 * (az - 0.005), torch.zeros_like(z)).mean(1)
        return per

    def nrm(v):
        return torch.nn.functional.normalize(v, p=2, dim=2)
    per = [None] * 13
    for h, (side, face) in enumerate(zip(SIDES, faces)):
        f = torch.from_numpy(face.astype(np.int64))
        cen = T(gt['center_' + side])
        pm, gm = leaves['pd_mesh_xyz_' + side] / 0.15, (T(gt['mesh_3d_' + side]) - cen) / 0.15
        pj, gj = leaves['pd_joint_xyz_' + side] / 0.15, (T(gt['joint_3d_' + side]) - cen) / 0.15
        per[0 + h] = sl1(leaves['pd_joint_uv_' + side], T(gt['joint_2d_' + side])[:, :, :2])
        per[2 + h] = sl1(leaves['pd_mesh_uv_' + side], T(gt['mesh_2d_' + side])[:, :, :2])
        per[4 + h], per[6 + h] = sl1(pj, gj), sl1(pm, gm)
        d = lambda c, a, b: torch.sqrt(((c[:, f[:, a]] - c[:, f[:, b]]) ** 2).sum(2) + 1e-12)  # noqa: E731
        per[8 + h] = torch.cat([(d(pm, a, b) - d(gm, a, b)).abs() for a, b in ((0, 1), (0, 2), (1, 2))], 1).mean(1)
        v1o, v2o, v3o = nrm(pm[:, f[:, 1]] - pm[:, f[:, 0]]), nrm(pm[:, f[:, 2]] - pm[:, f[:, 0]]), nrm(pm[:, f[:, 2]] - pm[:, f[:, 1]])
        ng = nrm(torch.cross(nrm(gm[:, f[:, 1]] - gm[:, f[:, 0]]), nrm(gm[:, f[:, 2]] - gm[:, f[:, 0]]), dim=2))
        per[10 + h] = torch.cat([(v * ng).sum(2).abs() for v in (v1o, v2o, v3o)], 1).mean(1)
    per[12] = sl1(leaves['pd_offset'], ((T(gt['center_right']) - T(gt['center_left'])) / 0.15)[:, 0])
    w = torch.tensor([case.coord_weight if (k < 8 or k == 12) else (1.0 if k < 10 else 0.1) for k in range(13)], dtype=torch.float32)
    sc = torch.stack(per, 1)
    terms = sc.mean(0) * w
    (terms * gout).sum().backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out['scratch'], out['out13'] = sc.detach().numpy().astype(np.float64), terms.detach().numpy()
    return out


# ===================================================================================================================== dense: cases
DenseCase = collections.namedtuple('DenseCase', 'name B S H W labels logits class_weight dense_weight gout')
DENSE_SIZES = ((1, 1), (3, 1), (1, 15), (1, 16), (1, 17), (7, 17), (2, 32), (1, 46), (1, 90), (8, 32), (1, 91), (16, 32), (2, 91), (65, 16), (129, 4))
DENSE_HW = ('same', (256, 256), (100, 100), (37, 37), (8, 8), (1, 1), (96, 64), (37, 100))
DENSE_LABELS = ('all', 'absent1', 'only2', 'single_first', 'single_last')
DENSE_LOGITS = ('normal', 'quant', 'equal', 'byte0', 'byte1', 'byte2', 'byte3', 'zero_err', 'big', 'denormal', 'negzero')
DENSE_CW = ((0.1, 0.45, 0.45), (1.0, 2.0, 3.0), (0.5, 0.0, 1.5))
DENSE_GOUT = (None, (0.75, 1.5, 2.25), (1.25, 0.0, 0.5))


@functools.lru_cache(maxsize=None)
def dense_cases():
    L = []

    def add(B, S, hw, lab, lg):
        i = len(L)
        H, W = (S, S) if hw == 'same' else hw
        if B * H * W > 400000:                                               # keep the targets small: the large batches take the small maps
            H, W = (8, 8) if i % 2 else (37, 20)
        cw = DENSE_CW[i % 3]                                                 # the zero weight sits on class 1: never the only class present
        L.append(DenseCase('%02d_b%d_s%d_%dx%d_%s_%s' % (i, B, S, H, W, lab, lg), B, S, H, W, lab, lg, cw, (1.0, 0.37)[i % 2], DENSE_GOUT[(i // 2) % 3]))
    for i, (B, S) in enumerate(DENSE_SIZES):
        add(B, S, DENSE_HW[i % len(DENSE_HW)], DENSE_LABELS[i % 5], DENSE_LOGITS[i % len(DENSE_LOGITS)])
    for i, lg in enumerate(DENSE_LOGITS):                                    # every logit class on both sides of 2048 and of 8192
        add(7, 17, DENSE_HW[(i + 3) % len(DENSE_HW)], DENSE_LABELS[(i + 2) % 5], lg)
        add(1, 91, DENSE_HW[(i + 5) % len(DENSE_HW)], 'all' if i % 2 else 'absent1', lg)
    for i, lab in enumerate(DENSE_LABELS):
        add(2, 91, DENSE_HW[i % len(DENSE_HW)], lab, ('normal', 'quant')[i % 2])
    add(1, 4, (1, 1), 'all', 'normal')
    add(1, 16, (8, 8), 'all', 'quant')
    add(2, 32, (256, 256), 'all', 'equal')
    add(1, 16, (100, 100), 'all', 'normal')                                  # the non-integer ratios 100 -> 16 and 37 -> 20
    add(2, 20, (37, 37), 'absent1', 'quant')
    return tuple(L)


@functools.lru_cache(maxsize=None)
def dense_inputs(case):
    rng, B, S, H, W = _rng('dense.' + case.name), case.B, case.S, case.H, case.W
    lab = {'all': (0, 1, 2), 'absent1': (0, 2), 'only2': (2,)}.get(case.labels)
    if lab is not None:
        gt_seg = rng.choice(lab, size=(B, 1, H, W)).astype(F32)
    else:                                                                    # one foreground pixel (class 1) at the first / last index of the batch
        gt_seg = np.zeros((B, 1, H, W), F32)
        if case.labels == 'single_first':
            gt_seg[0, 0, 0, 0] = 1
        else:
            gt_seg[-1, 0, _nearest_idx(H, S, None)[-1], _nearest_idx(W, S, None)[-1]] = 1      # the source pixel that the last output pixel takes
    shape = (B, 3, S, S)
    k = case.logits
    if k == 'normal':
        seg = rng.normal(0, 1.5, shape)
    elif k == 'quant':
        seg = np.round(rng.normal(0, 1.5, shape) * 2) / 2
    elif k == 'equal':
        seg = np.full(shape, 0.5)
    elif k.startswith('byte'):                                               # float bits differ in byte n only (and in the sign): radix pass n alone orders the background
        n = int(k[4])
        byte = rng.randint(0x30 if n == 3 else 0, 0x50 if n == 3 else 256, shape).astype(np.uint32)
        base = np.uint32(0x00400000 if n == 3 else 0x3F000000)
        if n == 2:
            byte &= np.uint32(0x7F)                                          # bit 23 belongs to the exponent byte
        bits = (base & ~np.uint32(0xFF << (8 * n))) | (byte << np.uint32(8 * n)) | (rng.randint(0, 2, shape).astype(np.uint32) << np.uint32(31))
        seg = bits.astype(np.uint32).view(F32)
    elif k == 'zero_err':                                                    # logit == fg on half the pixels: errors exactly 0, sign(0) = 0
        seg = rng.normal(0, 1.5, shape)
        labS = OL.interpolate_nearest(gt_seg, S).astype(np.int64)[:, 0]
        fg = np.stack([(labS == c) for c in range(3)], 1).astype(np.float64)
        seg = np.where(rng.rand(*shape) < 0.5, fg, seg)
    elif k == 'big':
        seg = rng.choice((-1e4, 1e4), size=shape) + rng.normal(0, 1.0, shape)
    elif k == 'denormal':
        seg = (rng.randint(1, 1 << 22, shape).astype(np.uint32) | (rng.randint(0, 2, shape).astype(np.uint32) << np.uint32(31))).view(F32)
    elif k == 'negzero':
        seg = np.where(rng.rand(*shape) < 0.5, -0.0, rng.choice((0.0, 1.0, 0.25), size=shape))
    else:
        raise KeyError(k)
    seg = np.ascontiguousarray(seg, F32)
    dense = rng.uniform(0, 1, shape).astype(F32)
    gt_dense = (rng.randint(0, 256, (B, 3, H, W)) / F32(255.0)).astype(F32)
    tgt = OL.interpolate_bilinear(gt_dense, S)
    m = rng.rand(*shape) < 0.4                                               # residuals under the knee, and a few exactly 0
    dense[m] = (tgt + rng.normal(0, 0.004, shape).astype(F32))[m]
    z = rng.rand(*shape) < 0.02
    dense[z] = tgt[z]
    for a in (seg, dense, gt_seg, gt_dense):
        a.setflags(write=False)
    return seg, dense, gt_seg, gt_dense


# ===================================================================================================================== dense: restatement
def _taps(n_in, S, defect):
    """F.interpolate(bilinear, align_corners=False) source taps in float32 (oracle/losses.py: interpolate_bilinear)"""
    src = (np.arange(S, dtype=F32) + F32(0.5)) * (F32(n_in) / F32(S)) - F32(0.5)
    if defect != 'bilinear_no_clamp_at_0':
        src = np.maximum(src, F32(0.0))
    src = src.astype(F32)
    i0 = np.maximum(np.floor(src), 0).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1.0) - l1).astype(F32), l1, np.abs(src).astype(np.float64)


def _nearest_idx(n_in, S, defect):
    x = np.arange(S, dtype=F32) * (F32(n_in) / F32(S))
    x = np.floor(x + F32(0.5)) if defect == 'nearest_by_rounding' else np.floor(x)
    return np.minimum(x.astype(np.int64), n_in - 1)


def _jaccard(fs, defect):
    """models/lovasz_loss.py:19-31 on the sorted foreground flags, float64; the kernel's pass length is LV_T LV_E = 8192"""
    P = fs.shape[0]
    G = fs.sum()
    cum = np.cumsum(fs)
    if defect == 'fg_carry_dropped':
        cum = np.concatenate([np.cumsum(fs[s:s + 8192]) for s in range(0, P, 8192)])
    J = 1.0 - (G - cum) / (G + (np.arange(1, P + 1) - cum))
    dJ = J.copy()
    dJ[1:] -= J[:-1]
    aJ = np.abs(J) + np.abs(1.0 - J)                                        # J = 1 - q: a float32 J carries u |q| too
    aJ[1:] += aJ[:-1].copy()
    if defect == 'prevJ_reset':
        dJ[8192::8192] = J[8192::8192]
    return dJ, aJ


def dense_eval(exact, case, defect=None):
    """Every output of dir_dense_losses_forward / _backward.  exact: float64 values and scales -> {name: (ref, S)}; else float32 in the kernel's
    documented order -> {name: value}."""
    seg, dense, gt_seg, gt_dense = dense_inputs(case)
    B, S, H, W = case.B, case.S, case.H, case.W
    P = B * S * S
    wd = np.float64 if exact else F32
    cw = np.asarray(case.class_weight, F32).astype(np.float64)
    dw = float(F32(case.dense_weight))
    go = np.ones(3) if case.gout is None else np.asarray(case.gout, F32).astype(np.float64)
    Wx = H if defect == 'H_used_for_W' else W
    iy, ix = _nearest_idx(H, S, defect), np.minimum(_nearest_idx(Wx, S, defect), W - 1)
    lab = np.clip(gt_seg[:, 0][:, iy[:, None], ix[None, :]].astype(np.int64), 0, 2)                  # [B, S, S]
    y0, y1, wy0, wy1, sy = _taps(H, S, defect)
    x0, x1, wx0, wx1, sx = _taps(Wx, S, defect)
    x0, x1 = np.minimum(x0, W - 1), np.minimum(x1, W - 1)
    g = gt_dense.astype(wd)
    if defect == 'x1_not_clamped':                                           # x0 + 1 past the row's end reads the next row's first element
        flat = g.reshape(B, 3, H * W)
        xn = np.minimum(_taps(Wx, S, None)[0], W - 1) + 1
        tap = lambda yy, xx, raw: flat[:, :, np.minimum(yy[:, None] * W + raw[None, :], H * W - 1)]  # noqa: E731
        g01, g11 = tap(y0, x1, xn), tap(y1, x1, xn)
    else:
        g01, g11 = g[..., y0[:, None], x1[None, :]], g[..., y1[:, None], x1[None, :]]
    g00, g10 = g[..., y0[:, None], x0[None, :]], g[..., y1[:, None], x0[None, :]]
    a0, a1, b0, b1 = (t.astype(wd) for t in (wx0, wx1, wy0[:, None], wy1[:, None]))
    tgt = b0 * (a0 * g00 + a1 * g01) + b1 * (a0 * g10 + a1 * g11)
    r0, r1 = np.abs(a0 * g00) + np.abs(a1 * g01), np.abs(a0 * g10) + np.abs(a1 * g11)
    # three roundings through the taps, and the weights' own derivation (src - floor(src): 3 u (src + 1) each)
    St = 3.0 * (np.abs(b0) * r0 + np.abs(b1) * r1) + 3.0 * (sx + 1.0) * (np.abs(b0) * (np.abs(g00) + np.abs(g01)) + np.abs(b1) * (np.abs(g10) + np.abs(g11))) \
        + 3.0 * (sy[:, None] + 1.0) * (r0 + r1)
    # ---- dense SmoothL1 (models/dir.py:566,568)
    x = dense.astype(wd)
    z = x - tgt
    az = np.abs(z)
    small = az < wd(F32(0.01))
    term = np.where(small, wd(0.5) * (z * z), wd(F32(0.01)) * (az - wd(F32(0.005))))
    dterm = np.where(small, z, wd(F32(0.01)) * np.sign(z))
    if exact:
        kd = float(F32(go[1])) * dw / (float(B) * 3.0 * S * S)
    else:
        kd = F32(go[1]) * F32(dw) / (F32(B) * F32(3.0) * F32(S) * F32(S))
    gdense = kd * dterm
    out_dense = term.astype(np.float64).mean() * dw
    # ---- cross entropy (models/dir.py:511,567)
    lg = seg.transpose(0, 2, 3, 1).reshape(P, 3)
    yv = lab.reshape(P)
    xs = lg.astype(np.float64)                                               # the kernels take exp, log and the softmax in double
    m = xs.max(1, keepdims=True)
    ex = np.exp(xs - m)
    es = ex.sum(1, keepdims=True)
    nll = (m[:, 0] + np.log(es[:, 0])) - xs[np.arange(P), yv]
    wv = cw[yv]
    out_seg = (wv * nll.astype(np.float64)).sum() / wv.sum() * 0.1 * dw
    sm = ex / es
    onehot = (yv[:, None] == np.arange(3)[None, :])
    gce = (go[0] * 0.1 * dw * wv / wv.sum())[:, None] * (sm.astype(np.float64) - onehot)
    # ---- lovasz_softmax(classes='present') on the raw logits (models/lovasz_loss.py:155-202)
    present = [c for c in range(3) if (yv == c).any() or defect == 'absent_class_counted']
    npres = len(present)
    glov, alov = np.zeros((P, 3)), np.zeros((P, 3))
    lsum = 0.0
    for c in range(3):
        fg = (yv == c)
        if not fg.any():
            continue
        err = np.abs(fg.astype(F32) - lg[:, c]).astype(F32)
        n = P - P % 2048 if defect == 'last_partial_tile_dropped' and P > 2048 else P
        if defect == 'tie_order_reversed':
            perm = (n - 1 - np.argsort(-err[:n][::-1], kind='stable'))
        else:
            perm = np.argsort(-err[:n], kind='stable')
        dJ, aJ = _jaccard(fg[perm].astype(np.float64), defect)
        alov[perm, c] = aJ * abs(go[2] * 0.1 * dw / npres)
        lsum += float((err[perm].astype(np.float64) * dJ).sum())
        dJ = dJ if exact else dJ.astype(F32).astype(np.float64)
        glov[perm, c] = np.sign(lg[perm, c].astype(np.float64) - fg[perm]) * dJ * (go[2] * 0.1 * dw / npres)
    out_lov = (lsum / npres if npres else 0.0) * 0.1 * dw
    gseg = gce + glov
    shp = lambda a: a.reshape(B, S, S, 3).transpose(0, 3, 1, 2)  # noqa: E731
    if not exact:
        return {'seg': F32(out_seg), 'dense': F32(out_dense), 'lovasz': F32(out_lov), 'grad_seg': shp(gseg).astype(F32), 'grad_dense': np.asarray(gdense, F32)}
    agce = np.abs(go[0] * 0.1 * dw * wv / wv.sum())[:, None] * (sm + onehot)
    S_el = np.where(small, az, float(F32(0.01))) * (St + az) + 3.0 * np.abs(term)
    S_gd = np.abs(gdense) + np.where(az <= 0.0101, kd * (np.abs(x) + St), 0.0)
    return {'seg': (out_seg, abs(out_seg)), 'lovasz': (out_lov, abs(out_lov)), 'dense': (out_dense, S_el.mean() * dw + abs(out_dense)),
            'grad_seg': (shp(gseg), shp(agce + alov) + np.abs(shp(gseg))), 'grad_seg_scan': (shp(gseg), shp(agce + np.abs(glov)) + np.abs(shp(gseg))),
            'grad_dense': (gdense, S_gd)}


def torch_dense(case):
    """(a): torch CPU float32 autograd through models/dir.py:562-569 (F.interpolate, CrossEntropyLoss(weight), SmoothL1Loss, lovasz_softmax with a
    stable descending sort -- the order the kernel promises)"""
    Fn = torch.nn.functional
    seg, dense, gt_seg, gt_dense = (torch.from_numpy(np.array(a)) for a in dense_inputs(case))
    seg.requires_grad_(True); dense.requires_grad_(True)
    S = case.S
    lab = Fn.interpolate(gt_seg, size=(S, S), mode='nearest').long()[:, 0].clamp(0, 2)
    tgt = Fn.interpolate(gt_dense, size=(S, S), mode='bilinear', align_corners=False)
    l_seg = Fn.cross_entropy(seg, lab, weight=torch.tensor(case.class_weight, dtype=torch.float32)) * 0.1 * case.dense_weight
    z = (dense - tgt).reshape(case.B, -1)
    az, small = z.abs(), z.abs() < 0.01
    l_dense = (torch.where(small, 0.5 * z * z, torch.zeros_like(z)).mean(1) + torch.where(~small, 0.01 * (az - 0.005), torch.zeros_like(z)).mean(1)).mean() * case.dense_weight
    pr, yv = seg.permute(0, 2, 3, 1).reshape(-1, 3), lab.reshape(-1)
    losses = []
    for c in range(3):
        fg = (yv == c).float()
        if fg.sum() == 0:
            continue
        err = (fg - pr[:, c]).abs()
        es, perm = torch.sort(err, dim=0, descending=True, stable=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1 - fs).cumsum(0))
        if fs.numel() > 1:
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    l_lov = (torch.stack(losses).mean() if losses else torch.zeros(())) * 0.1 * case.dense_weight
    go = (1.0, 1.0, 1.0) if case.gout is None else case.gout
    (go[0] * l_seg + go[1] * l_dense + go[2] * l_lov).backward()
    return {'seg': l_seg.item(), 'dense': l_dense.item(), 'lovasz': l_lov.item(), 'grad_seg': seg.grad.numpy(), 'grad_dense': dense.grad.numpy()}


# ===================================================================================================================== gate
def units(got, ref, S, widen=None, mask=None, c=None, f32_out=True):
    """c None: the largest |got - ref| in units of 2^-24 S over `mask` (what RATIOS records).  c given: the largest |got - ref| / tolerance,
    tolerance = c 2^-24 S + widen + half an ulp of a float32 output (2^-24 |ref|) + 2^-149; inf if an element is not finite"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    d = np.abs(got - ref)
    if widen is not None:
        d = np.maximum(d - widen, 0.0)
    r = d / (U * S + TINY) if c is None else d / (c * U * S + (U * np.abs(ref) if f32_out else 0.0) + TINY)
    if mask is not None:
        r = np.where(mask, r, 0.0)
    return float(np.max(r, initial=0.0))


@functools.lru_cache(maxsize=None)
def stage_reference(case):
    """{name: (ref64, S, widen, band)} of every output"""
    e = stage_eval(A64, case)
    out = {}
    for k in ('scratch', 'out13') + STAGE_GRADS:
        v = e[k]
        out[k] = (v.v, v.e / U, e.get('widen:' + k), e.get('band:' + k))
    return out


def stage_check(case, got, ref=None, what=''):
    """got: {name: array}.  Returns {kind: worst ratio / c}; raises AssertionError naming the first failures.  Degenerate cases: finite everywhere,
    the gate off the band."""
    ref = ref or stage_reference(case)
    worst, bad = {}, []
    for name, (r, S, widen, band) in ref.items():
        g = np.asarray(got[name], np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), '%s %s %s: not finite' % (what, case.name, name)
        mask = None if band is None or not case.degenerate else ~band
        for k in (range(13) if name in ('scratch', 'out13') else (None,)):
            sel = (Ellipsis, k) if k is not None else Ellipsis
            kind = stage_kind(name, k)
            u = units(g[sel], r[sel], S[sel], None if widen is None else widen[sel], None if mask is None else mask[sel], CONSTANTS[kind], name != 'scratch')
            worst[kind] = max(worst.get(kind, 0.0), u)
            if not u <= 1.0:
                bad.append('%s %s %s%s: %.4g x the bound (c = %.4g)' % (what, case.name, name, '' if k is None else '[%d]' % k, u, CONSTANTS[kind]))
    assert not bad, '\n'.join(bad[:20])
    return worst


def band_fraction(case, ref=None):
    ref = ref or stage_reference(case)
    n = sum(ref[k][0].size for k in STAGE_GRADS)
    return sum(int(ref[k][3].sum()) for k in STAGE_GRADS if ref[k][3] is not None) / float(n)


DENSE_OUTPUTS = ('seg', 'dense', 'lovasz', 'grad_seg', 'grad_dense')
DENSE_KINDS = DENSE_OUTPUTS + ('grad_seg_scan',)                             # gates; grad_seg_scan reads the output grad_seg
FLOAT64_SCAN_ONLY = ('grad_seg_scan',)                                       # gates that a float32 Jaccard scan (torch's) is not asked to meet


def _out(kind):
    return 'grad_seg' if kind == 'grad_seg_scan' else kind


@functools.lru_cache(maxsize=None)
def dense_reference(case):
    """{name: (ref64, S)}"""
    return dense_eval(True, case)


@functools.lru_cache(maxsize=None)
def _clean32(family, case):
    return stage_eval(A32, case) if family == 'stage' else dense_eval(False, case)


def dense_check(case, got, ref=None, what='', float64_scan=True):
    """float64_scan False: the gates a float32 Jaccard scan can meet (what torch's float32 autograd is held to)"""
    ref = ref or dense_reference(case)
    worst, bad = {}, []
    for k in DENSE_KINDS:
        if k in FLOAT64_SCAN_ONLY and not float64_scan:
            continue
        u = units(got[_out(k)], ref[k][0], ref[k][1], c=CONSTANTS[k])
        worst[k] = u
        if not u <= 1.0:
            bad.append('%s %s %s: %.4g x the bound (c = %.4g)' % (what, case.name, k, u, CONSTANTS[k]))
    assert not bad, '\n'.join(bad)
    return worst


# ===================================================================================================================== constants
def measure_stage():
    """{kind: {'torch': ratio, 'numpy': ratio}} over the non-degenerate list, off the band"""
    R = {}
    for case in stage_cases():
        if case.degenerate:
            continue
        ref = stage_reference(case)
        for tag, got in (('torch', torch_stage(case)), ('numpy', _clean32('stage', case))):
            for name, (r, S, widen, band) in ref.items():
                g = np.asarray(got[name], np.float64).reshape(r.shape)
                for k in (range(13) if name in ('scratch', 'out13') else (None,)):
                    sel = (Ellipsis, k) if k is not None else Ellipsis
                    u = units(g[sel], r[sel], S[sel], None, None if band is None else ~band[sel])
                    d = R.setdefault(stage_kind(name, k), {'torch': 0.0, 'numpy': 0.0})
                    d[tag] = max(d[tag], u)
    return R


def measure_dense():
    R = {k: ({'numpy': 0.0} if k in FLOAT64_SCAN_ONLY else {'torch': 0.0, 'numpy': 0.0}) for k in DENSE_KINDS}
    for case in dense_cases():
        ref = dense_reference(case)
        for tag, got in (('torch', torch_dense(case)), ('numpy', _clean32('dense', case))):
            for k in DENSE_KINDS:
                if tag in R[k]:
                    R[k][tag] = max(R[k][tag], units(got[_out(k)], ref[k][0], ref[k][1]))
    return R


# measured by measure_stage() / measure_dense() (CPU float32 references, never the kernels; torch 2.10.0, one thread), recorded 25 % above the
# measurement: torch's float32 reductions (log-sum-exp, cumsum, dot) move a little with the build and its SIMD path
RATIOS = {
    'seg':            {'torch': 9.63, 'numpy': 1.16},
    'dense':          {'torch': 0.214, 'numpy': 0.0284},
    'lovasz':         {'torch': 6.6, 'numpy': 0.806},
    'grad_seg':       {'torch': 20.0, 'numpy': 0.624},
    'grad_dense':     {'torch': 1.11, 'numpy': 1.11},
    'grad_seg_scan':  {'numpy': 1.1},
    'scratch_sl1':    {'torch': 1.32, 'numpy': 0.48},
    'scratch_edge':   {'torch': 0.165, 'numpy': 0.112},
    'scratch_normal': {'torch': 0.0277, 'numpy': 0.0307},
    'out13_sl1':      {'torch': 0.698, 'numpy': 0.348},
    'out13_edge':     {'torch': 0.0448, 'numpy': 0.0448},
    'out13_normal':   {'torch': 0.0276, 'numpy': 0.0276},
    'g_joint_uv':     {'torch': 1.03, 'numpy': 1.02},
    'g_mesh_uv':      {'torch': 1.29, 'numpy': 0.944},
    'g_joint_xyz':    {'torch': 1.03, 'numpy': 1.03},
    'g_mesh_xyz':     {'torch': 1.04, 'numpy': 1.04},
    'g_offset':       {'torch': 0.817, 'numpy': 0.848},
}
CONSTANTS = {k: 4.0 * max(v.values()) for k, v in RATIOS.items()}


# ===================================================================================================================== defects
Defect = collections.namedtuple('Defect', 'name family what')
DEFECTS = (
    Defect('tie_order_reversed', 'dense', 'equal keys leave the sort in descending pixel order'),
    Defect('fg_carry_dropped', 'dense', 'the foreground count restarts at every 8192 sorted elements'),
    Defect('prevJ_reset', 'dense', 'J of the previous pass forgotten: the first element of a pass gets J, not J - J_prev'),
    Defect('last_partial_tile_dropped', 'dense', 'the elements after the last full 2048-tile never reach the scan'),
    Defect('nearest_by_rounding', 'dense', 'nearest source index by rounding instead of floor'),
    Defect('bilinear_no_clamp_at_0', 'dense', 'negative source coordinates extrapolate instead of clamping'),
    Defect('x1_not_clamped', 'dense', 'x0 + 1 runs past the row'),
    Defect('absent_class_counted', 'dense', 'n_present = 3 whatever the labels'),
    Defect('H_used_for_W', 'dense', 'the column scale taken from H'),
    Defect('edge_normal_swapped', 'stage', 'grad_out slots 8 + h and 10 + h exchanged'),
    Defect('left_right_swapped', 'stage', 'grad_out slot k + h read at k + 1 - h'),
    Defect('c2_stride_2', 'stage', 'the 2-D targets read at stride 2 whatever c2'),
    Defect('last_csr_corner_skipped', 'stage', "a vertex's last corner left out of its sum"),
    Defect('eps_outside_sqrt', 'stage', 'sqrt(sumsq) + 1e-12 for sqrt(sumsq + 1e-12)'),
    Defect('normal_from_prediction', 'stage', 'the face normal taken from the predicted mesh'),
    Defect('offset_without_1_over_B', 'stage', '1 / B missing from the offset gradient'),
)
# defects no float32 gate can see on ANY case: none
EQUIVALENT = {}
# cases on which a defect changes bits of the clean float32 result and the gate accepts it all the same, with the reason no float32 gate can do otherwise;
# on every other case that a defect changes, the gate must reject it (tests/test_loss_cases_ref.py)
_ONE_SOURCE_PIXEL = 'H = W = 1: all four taps read the one source pixel, so unclamped weights still sum to 1 and the target moves by its own rounding only'
_ONE_EDGE_OF_MANY = ('the one 1e-7 edge is 1 of >= 765 in a float64 mean whose float32 elements carry u len ~ 3e-8 each: the move, 9e-7 / (3 F), is below what another '
                     'valid float32 order gives; at its two vertices the normal term (1 / |e| = 1e7) sets |g| and the edge part is below an ulp of it.  f1_tiny rejects')
NOT_REJECTED = {
    'bilinear_no_clamp_at_0': {n: _ONE_SOURCE_PIXEL for n in ('13_b65_s16_1x1_single_first_equal', '19_b7_s17_1x1_single_last_equal', '32_b1_s91_1x1_absent1_big',
                                                              '42_b1_s4_1x1_all_normal')},
    'eps_outside_sqrt': {n: _ONE_EDGE_OF_MANY for n in ('b1_c5_proj_gout', 'b3_c5', 'b64_c3', 'b65_c5', 'b129_c5', 'f255', 'fmax')},
}
# defects that the gates of tests/test_gpu_loss.py (close(): 1e-5 max(|want|, 1e-3) on the scalars; 2e-5 of each gradient tensor's maximum), pointed at THIS
# list, accept on at least one case that they change -- measured by tests/test_loss_cases_ref.py
OLD_GATES_ACCEPT = ('tie_order_reversed', 'bilinear_no_clamp_at_0')
# defects that the old SUITE could not see whatever its gates, because no case of it varied what they touch
OLD_SUITE_BLIND = {
    'edge_normal_swapped': 'grad_out was checked on pd_joint_uv_left (slot 0) only',
    'left_right_swapped': 'grad_out was checked on pd_joint_uv_left (slot 0) only',
    'c2_stride_2': 'the backward ran at c2 = 3 only, and its forward c2 = 2 case is the stride the defect assumes',
    'H_used_for_W': 'H == W in every dense case',
    'x1_not_clamped': 'H >= S in every dense case: x0 + 1 never left the row',
    'prevJ_reset': 'the per-pixel Lovasz gradient was held to 2e-5 of the maximum at P = 2048 ... 65536 with random logits only',
}


def old_gates_accept(got, ref):
    """the max-norm gates of tests/test_gpu_loss.py on {name: array} against {name: float64 reference}"""
    for k, r in ref.items():
        g, r = np.asarray(got[k], np.float64).reshape(np.shape(r)), np.asarray(r, np.float64)
        if k in ('seg', 'dense', 'lovasz', 'out13'):
            if not (np.abs(g - r) <= 1e-5 * np.maximum(np.abs(r), 1e-3)).all():
                return False
        elif k != 'scratch':                                                 # the per-sample table had no gate
            if not np.abs(g - r).max() <= 2e-5 * np.abs(r).max():
                return False
    return True


def defect_report(d):
    """(names of the cases whose float32 result the defect changes in any bit, names of those that the gate accepts all the same, whether the old
    gates accept a changed case somewhere)"""
    moved, accepted, old_ok = [], [], False
    for case in (stage_cases() if d.family == 'stage' else dense_cases()):
        if d.family == 'stage':
            if case.degenerate:
                continue
            clean, bad, ref = _clean32('stage', case), stage_eval(A32, case, d.name), stage_reference(case)
            names, check = ('scratch', 'out13') + STAGE_GRADS, stage_check
        else:
            clean, bad, ref = _clean32('dense', case), dense_eval(False, case, d.name), dense_reference(case)
            names, check = DENSE_OUTPUTS, dense_check
        if all(np.array_equal(np.asarray(clean[k]), np.asarray(bad[k])) for k in names):
            continue
        moved.append(case.name)
        try:
            check(case, bad, ref)
            accepted.append(case.name)
        except AssertionError:
            pass
        old_ok = old_ok or old_gates_accept(bad, {k: ref[k][0] for k in names})
    return moved, accepted, old_ok


def CONSTANTS_OF(name, S):
    """c 2^-24 S + tiny per element of a stage output (the 13 slots of scratch / out13 take their term's constant)"""
    S = np.asarray(S, np.float64)
    if name in ('scratch', 'out13'):
        c = np.array([CONSTANTS[stage_kind(name, k)] for k in range(13)])
        return c * U * S + TINY
    return CONSTANTS[stage_kind(name)] * U * S + TINY
