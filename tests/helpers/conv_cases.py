"""Edge descriptors of the forward convolution family, operands with scale structure, a float64 reference and a per-element check.
CPU only (torch CPU + numpy): tests/test_conv_cases_ref.py proves the pieces here, tests/test_gpu_conv_sweep.py points the kernels at them.

cases(kind)                      the descriptor list of one kind, grouped in CLASSES (Cin follows the kind's slab: 32 channels for the
                                 fp32-sized kinds, 64 for the 16-bit ones, so `nk` -- the number of K slabs -- is the same in every kind)
make(case, kind, seed)           operands +-(0.5 + U[0,1)) 2^e, 5 % exact zeros: activations e = e_c[cin] + g[b,y,x], weights e = -e_c[cin] + f[cout]
                                 (times 1 / sqrt(K)), so every input channel weighs the same in every output while outputs span ~2^24
reference(case, operands, kind)  (ref, S) in float64: the exact result on the operands as stored, S = |scale| conv(|a|, |w|) + |shift| + |residual|
check(got, ref, S, case, kind)   every element: |got - ref| <= acc + round_T(ref, acc), acc = c(kind) sqrt(K) 2^-24 S; canaries bit-unchanged

Kinds: 'f32' exact fp32, 'bf16' / 'f16s' 16-bit storage, 'f16x3' / 'f16' fp32 tensors on f16 arithmetic (split precision / hi parts only)."""
import collections
import math
import zlib

import numpy as np
import torch

KINDS = ('f32', 'bf16', 'f16s', 'f16x3', 'f16')
HALF_KINDS = ('bf16', 'f16s')
BK = {'f32': 32, 'f16x3': 32, 'f16': 32, 'bf16': 64, 'f16s': 64}           # K slab = the Cin granule of dir_conv2d_forward
EPC = {'f32': 4, 'f16x3': 4, 'f16': 4, 'bf16': 8, 'f16s': 8}               # elements per 16 bytes of input
STORE = {'f32': torch.float32, 'f16x3': torch.float32, 'f16': torch.float32, 'bf16': torch.bfloat16, 'f16s': torch.float16}
CLASSES = ('m_tails', 'n_tails', 'k_slabs', 'geometry', 'halo', 'slices', 'epilogue', 'dual', 'splitk')
COUNTS = {'m_tails': 13, 'n_tails': 16, 'k_slabs': 16, 'geometry': 19, 'halo': 9, 'slices': 9, 'epilogue': 26, 'dual': 6, 'splitk': 6}

# c(kind) of the accumulation bound: 4 x the largest |got - ref| / (sqrt(K) 2^-24 S) the sweep measured on the MI355X with the check off
# (tests/test_gpu_conv_sweep.py's docstring has the measured ratios); check() caps it per descriptor, see c_eff
C = {'f32': 2.13, 'bf16': 0.434, 'f16s': 0.448, 'f16x3': 1.80, 'f16': 0.744}        # 4 x (0.533, 0.1085, 0.112, 0.451, 0.186)

_FIELDS = ('name cls B H W Cin Cout kh kw stride pad in_cs in_coff out_cs out_coff res_cs res_coff scale shift relu residual pre neg_scale '
           'out Cin2 H2 W2 stride2 splits')


class Case(collections.namedtuple('Case', _FIELDS)):
    """one descriptor.  pre: None | 'relu' | 'linear' (pre-activation with / without its ReLU); out: 'same' (the storage type) | 'f32';
    Cin2 > 0: dir_conv2d_dual_forward's second source [B, H2, W2, Cin2] read at stride2; splits > 1: dir_conv2d_splitk_forward"""
    __slots__ = ()
    Ho = property(lambda s: (s.H + 2 * s.pad - s.kh) // s.stride + 1)
    Wo = property(lambda s: (s.W + 2 * s.pad - s.kw) // s.stride + 1)
    M = property(lambda s: s.B * s.Ho * s.Wo)
    K = property(lambda s: s.kh * s.kw * s.Cin + s.Cin2)

    def nk(self, kind):
        return self.K // BK[kind]

    def out_dtype(self, kind):
        return torch.float32 if self.out == 'f32' else STORE[kind]

    def __str__(self):
        return self.name


def _mk(kind, cls, label, B, H, W, nkc, Cout, k=1, stride=1, pad=0, in_extra=(0, 0), out_extra=(0, 0), res_extra=(0, 0), scale=True, shift=True,
        relu=True, residual=False, pre=None, neg_scale=False, out='same', dual=None, splits=1):
    kh, kw = (k, k) if isinstance(k, int) else k
    Cin = nkc * BK[kind]
    Cin2, H2, W2, s2 = (dual[0] * BK[kind], dual[1], dual[2], dual[3]) if dual else (0, 0, 0, 0)
    return Case('%s-%s' % (cls, label), cls, B, H, W, Cin, Cout, kh, kw, stride, pad, in_extra[0] + Cin + in_extra[1], in_extra[0],
                out_extra[0] + Cout + out_extra[1], out_extra[0], res_extra[0] + Cout + res_extra[1], res_extra[0], scale, shift, relu, residual,
                pre, neg_scale, out, Cin2, H2, W2, s2, splits)


M_TAIL_VALUES = (1, 63, 64, 65, 127, 128, 135, 256, 257)
N_TAIL_VALUES = (1, 3, 6, 8, 24, 33, 63, 64, 65, 72, 127, 129, 136, 255, 257, 264)
NK_VALUES = (1, 2, 3, 4, 5, 8, 9, 11, 12, 13)
GEOMETRY_KSP = ((1, 1, 0), (1, 1, 1), (1, 2, 0), (3, 1, 0), (3, 1, 1), (3, 1, 2), (3, 2, 0), (3, 2, 1), (3, 3, 1))
GEOMETRY_KERNELS = (((1, 3), 0), ((3, 1), 0), ((2, 2), 0), ((4, 4), 0), ((5, 5), 2))


def cases(kind, cls=None):
    """the explicit descriptor list of `kind` (of one class if cls is given); split-K exists for the 16-bit kinds only (dir_conv2d_splitk_forward)"""
    assert kind in KINDS
    mk = lambda *a, **k: _mk(kind, *a, **k)      # noqa: E731
    L = []
    # ---- M tails: B x Ho x Wo around the 64 / 128 / 256-row tiles; Cout = 136 crosses one 128-wide N tile and keeps the vector epilogue
    shapes = [(1, 1, 1, 1), (63, 1, 7, 9), (64, 1, 8, 8), (65, 1, 5, 13), (127, 1, 1, 127), (128, 2, 8, 8), (135, 1, 9, 15), (256, 1, 16, 16),
              (257, 1, 1, 257)]
    for i, (m, B, H, W) in enumerate(shapes):
        k3 = i % 2 == 1
        L.append(mk('m_tails', 'M%d_%dx%dx%d_k%d' % (m, B, H, W, 3 if k3 else 1), B, H, W, 1 if k3 else 3, 136, 3 if k3 else 1, 1, 1 if k3 else 0,
                    out='f32' if m in (65, 257) else 'same'))
    L.append(mk('m_tails', 'W1_1x257x1_k3', 1, 257, 1, 1, 136, 3, 1, 1))
    L.append(mk('m_tails', 'H1_1x1x7_k3', 1, 1, 7, 1, 136, 3, 1, 1))
    L.append(mk('m_tails', 'H1_1x1x7_k1', 1, 1, 7, 3, 136))
    L.append(mk('m_tails', 'B5_4x4_k3', 5, 4, 4, 1, 136, 3, 1, 1))                     # one 64-row tile spans four images
    # ---- N tails: Cout across the 64 / 128 / 256 tile edges, vector (Cout % 8 == 0) and scalar epilogue
    for i, n in enumerate(N_TAIL_VALUES):
        k3 = i % 2 == 1
        L.append(mk('n_tails', 'N%d_k%d' % (n, 3 if k3 else 1), 1, 9, 15, 1 if k3 else 3, n, 3 if k3 else 1, 1, 1 if k3 else 0,
                    out='f32' if n in (6, 65, 136) else 'same'))
    # ---- K: slab counts around nk <= 4, DIR_PIPE_MIN_NK = 8, DIR_RING_MIN_NK = 12 and below the ring prologue
    for i, nk in enumerate(NK_VALUES):
        L.append(mk('k_slabs', 'nk%d_1x1' % nk, 1 + i % 2, 8, 8, nk, 128, out='f32' if nk in (2, 11) else 'same'))
    L.append(mk('k_slabs', 'nk9_3x3', 2, 8, 8, 1, 128, 3, 1, 1))
    L.append(mk('k_slabs', 'nk3_1x3', 1, 8, 10, 1, 128, (1, 3)))
    L.append(mk('k_slabs', 'nk12_1x3', 2, 8, 10, 4, 128, (1, 3)))
    L.append(mk('k_slabs', 'nk4_2x2', 1, 9, 9, 1, 128, 2))
    L.append(mk('k_slabs', 'nk8_2x2', 2, 9, 9, 2, 128, 2))
    L.append(mk('k_slabs', 'nk36_3x3', 1, 8, 8, 4, 128, 3, 1, 1))                            # the longest reduction: K = 2304 in the 16-bit kinds
    # ---- geometry: (k, stride, pad) on an odd map, stride 2 on an even one, non-square and even kernels, maps smaller than the kernel
    for k, s, p in GEOMETRY_KSP:
        L.append(mk('geometry', 'k%ds%dp%d_9x11' % (k, s, p), 1, 9, 11, 1, 40, k, s, p))
    for k, s, p in ((1, 2, 0), (3, 2, 0), (3, 2, 1)):
        L.append(mk('geometry', 'k%ds%dp%d_8x10' % (k, s, p), 2, 8, 10, 1, 40, k, s, p))
    for (kh, kw), p in GEOMETRY_KERNELS:
        L.append(mk('geometry', 'k%dx%dp%d_9x11' % (kh, kw, p), 1, 9, 11, 1, 40, (kh, kw), 1, p))
    L.append(mk('geometry', 'k3s1p1_1x1map', 3, 1, 1, 1, 40, 3, 1, 1))
    L.append(mk('geometry', 'k3s1p1_2x2map', 3, 2, 2, 1, 40, 3, 1, 1))
    # ---- halo geometry (patch_geometry in conv_pipe.hip): stride-1 3x3 at widths that divide 256 and that do not, rows > Ho with fewer
    # images than segments, Ho % rows != 0, a patch past PATCH_MAX_ROWS
    for label, B, H, W in (('8x8_B1', 1, 8, 8), ('8x8_B3', 3, 8, 8), ('16x16', 1, 16, 16), ('8x32', 1, 8, 32), ('4x32', 1, 4, 32), ('9x9', 1, 9, 9),
                           ('12x12', 1, 12, 12), ('12x16', 1, 12, 16), ('6x32', 1, 6, 32)):
        L.append(mk('halo', label, B, H, W, 1, 128, 3, 1, 1))
    # ---- slices: channel strides and offsets of input, output (canary channels on both sides) and residual
    L.append(mk('slices', 'in', 2, 7, 9, 1, 40, 3, 1, 1, in_extra=(16, 24)))
    L.append(mk('slices', 'out', 2, 7, 9, 1, 40, 3, 1, 1, out_extra=(8, 16)))
    L.append(mk('slices', 'res', 2, 7, 9, 1, 40, 3, 1, 1, residual=True, res_extra=(8, 8)))
    L.append(mk('slices', 'all_s2', 2, 7, 9, 1, 40, 3, 2, 1, in_extra=(8, 8), out_extra=(16, 8), residual=True, res_extra=(24, 8)))
    L.append(mk('slices', 'f32_out_off3', 2, 7, 9, 1, 40, 3, 1, 1, out_extra=(3, 2), out='f32'))          # scalar epilogue: offset % 4 != 0
    L.append(mk('slices', 'f32_res_off2', 2, 7, 9, 1, 40, 3, 1, 1, residual=True, res_extra=(2, 1), out='f32'))
    L.append(mk('slices', 'out_off4', 2, 7, 9, 1, 40, 3, 1, 1, out_extra=(4, 4)))                         # scalar for 16-bit, vector for fp32
    L.append(mk('slices', 'tail33_s2_k1', 2, 7, 9, 2, 33, 1, 2, 0, in_extra=(8, 0), out_extra=(5, 3), residual=True, res_extra=(1, 2)))
    L.append(mk('slices', 'k1_128_8x8', 2, 8, 8, 2, 128, in_extra=(16, 8), out_extra=(8, 24), residual=True, res_extra=(8, 8)))
    # ---- epilogue: every subset of {scale, shift, relu, residual}, negative scales before the ReLU, pre-activation over padding, fp32 output
    for bits in range(16):
        sc, sh, rl, rs = bool(bits & 1), bool(bits & 2), bool(bits & 4), bool(bits & 8)
        L.append(mk('epilogue', 'sub_%s%s%s%s' % ('S' if sc else '-', 'B' if sh else '-', 'R' if rl else '-', 'A' if rs else '-'), 1, 7, 9, 1, 40, 3, 1, 1,
                    scale=sc, shift=sh, relu=rl, residual=rs))
    L.append(mk('epilogue', 'neg_scale', 1, 7, 9, 1, 40, 3, 1, 1, neg_scale=True))
    L.append(mk('epilogue', 'neg_scale_res', 1, 7, 9, 1, 40, 3, 1, 1, neg_scale=True, residual=True))
    L.append(mk('epilogue', 'pre_relu_k3p1', 1, 7, 9, 1, 40, 3, 1, 1, pre='relu'))
    L.append(mk('epilogue', 'pre_linear_k3p1', 1, 7, 9, 1, 40, 3, 1, 1, pre='linear'))
    L.append(mk('epilogue', 'pre_relu_k3p2', 1, 7, 9, 1, 40, 3, 1, 2, pre='relu'))
    L.append(mk('epilogue', 'pre_linear_k1p1', 1, 7, 9, 2, 40, 1, 1, 1, pre='linear'))
    L.append(mk('epilogue', 'pre_relu_k1p0', 1, 7, 9, 2, 40, 1, 1, 0, pre='relu', residual=True))
    L.append(mk('epilogue', 'f32_out_all', 1, 7, 9, 1, 40, 3, 1, 1, residual=True, out='f32'))
    L.append(mk('epilogue', 'f32_out_res', 1, 7, 9, 1, 40, 3, 1, 1, scale=False, shift=False, relu=False, residual=True, out='f32'))
    L.append(mk('epilogue', 'f32_out_plain', 1, 7, 9, 1, 40, 3, 1, 1, scale=False, shift=False, relu=False, out='f32'))
    # ---- dual source (dir_conv2d_dual_forward): relu(conv1x1(y) + conv1x1_stride2(x2) + shift); H2 = 2 Ho - 1 and 2 Ho, Cin2 != Cin, ragged Cout
    L.append(mk('dual', 's2_odd9', 2, 5, 5, 1, 64, scale=False, dual=(2, 9, 9, 2)))
    L.append(mk('dual', 's2_even10', 2, 5, 5, 1, 64, scale=False, dual=(2, 10, 10, 2)))
    L.append(mk('dual', 's2_9x10_N33', 2, 5, 5, 2, 33, scale=False, dual=(1, 9, 10, 2)))
    L.append(mk('dual', 's1_N130', 1, 7, 9, 1, 130, scale=False, relu=False, dual=(1, 7, 9, 1)))
    L.append(mk('dual', 's2_M192_N136', 3, 8, 8, 3, 136, scale=False, dual=(2, 16, 16, 2)))
    L.append(mk('dual', 's3_N6', 2, 4, 4, 1, 6, scale=False, dual=(1, 10, 10, 3)))
    # ---- split-K (dir_conv2d_splitk_forward, 16-bit -> 16-bit): splits 2 / 3 / 16 on slab counts they do not divide, ragged M and N
    if kind in HALF_KINDS:
        L.append(mk('splitk', 's2_nk9', 1, 9, 15, 1, 136, 3, 1, 1, splits=2))
        L.append(mk('splitk', 's3_nk5', 1, 9, 15, 5, 72, splits=3))
        L.append(mk('splitk', 's2_nk5_res', 1, 9, 15, 5, 200, splits=2, residual=True))
        L.append(mk('splitk', 's16_nk17', 1, 9, 15, 17, 136, splits=16))
        L.append(mk('splitk', 's16_nk18_3x3', 2, 8, 8, 2, 128, 3, 1, 1, splits=16))
        L.append(mk('splitk', 's3_nk4_pre', 1, 9, 15, 4, 136, splits=3, pre='relu'))
    assert len({c.name for c in L}) == len(L)
    return [c for c in L if cls is None or c.cls == cls]


def classes(kind):
    return [c for c in CLASSES if c != 'splitk' or kind in HALF_KINDS]


# ---------------------------------------------------------------------------------------------------------------- which kernel is expected
# Kernel families the sweep tallies from the launch log, and the classes meant to reach each (on at least three descriptors).  '16' = the 16-bit
# kinds, 'x' = f16x3 / f16 with pre-split activations, '32' = exact fp32 and f16x3 / f16 without the pre-split pass (four-wave kernel only).
FAMILIES = ('igemm', 'igemm_ring', 'pipe', 'patch', 'big', 'pipe8', 'stream', 'as')
EXPECTED = {
    'm_tails': {'16': ('igemm', 'igemm_ring', 'pipe', 'big', 'pipe8'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'n_tails': {'16': ('igemm', 'igemm_ring', 'pipe', 'pipe8'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'k_slabs': {'16': ('igemm', 'igemm_ring', 'pipe', 'pipe8', 'stream', 'as'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'geometry': {'16': ('igemm', 'igemm_ring', 'pipe', 'pipe8'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'halo': {'16': ('igemm', 'igemm_ring', 'pipe', 'patch', 'pipe8', 'as'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'slices': {'16': ('igemm', 'igemm_ring', 'pipe'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'epilogue': {'16': ('igemm', 'igemm_ring', 'pipe', 'pipe8'), 'x': ('igemm', 'igemm_ring', 'pipe'), '32': ('igemm', 'igemm_ring')},
    'dual': {'16': ('igemm',), 'x': ('igemm',), '32': ('igemm',)},
    'splitk': {'16': ('igemm',)},
}
PATCH_MAX_ROWS = 400                     # conv_pipe.hip


def patch_expected(case, variant):
    """patch_geometry (conv_pipe.hip) restated: does the halo-reuse kernel take this descriptor under DIR_CONV_VARIANT 12 / 13 / 14?  Everything it
    refuses is served by the pipelined kernel of the same tile, or by the four-wave kernel where the pipelined one does not apply either."""
    bm = 128 if variant == 13 else 256
    ntaps = case.kh * case.kw
    if case.pre or case.stride != 1 or ntaps < 4 or bm % case.Wo:
        return False
    rows = bm // case.Wo
    if rows <= case.Ho:
        if case.Ho % rows:
            return False
        nseg, rows_seg = 1, rows
    else:
        if rows % case.Ho:
            return False
        nseg, rows_seg = rows // case.Ho, case.Ho
    npr = nseg * (rows_seg + case.kh - 1) * (case.Wo + case.kw - 1)
    return npr <= PATCH_MAX_ROWS and (npr + 63) // 64 <= ntaps - 1


def vector_epilogue(case, kind):
    """conv_forward's `vec`: every output / residual row segment 16-byte aligned (what the pipelined, 256 x 256 and eight-wave kernels need)"""
    epo = 4 if case.out_dtype(kind) == torch.float32 else 8
    ok = case.Cout % epo == 0 and case.out_cs % epo == 0 and case.out_coff % epo == 0
    return ok and (not case.residual or (case.res_cs % epo == 0 and case.res_coff % epo == 0))


# ------------------------------------------------------------------------------------------------------------------------------- operands
def _round(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt).float().numpy()


def _vals(rng, e):
    e = np.asarray(e, np.float64)
    v = (rng.integers(0, 2, e.shape) * 2 - 1) * (0.5 + rng.random(e.shape)) * np.exp2(e)
    v[rng.random(e.shape) < 0.05] = 0.0
    return v


def _pow2_floor_exp(a):
    return math.frexp(float(a))[1]          # a = m 2^e, m in [0.5, 1)


def make(case, kind, seed=0):
    """-> dict of float32 numpy operands (NCHW / OIHW), already rounded to the kind's storage type: x, w, scale, shift, res, ps, pb, x2, w2 (None
    where the descriptor has none), e_c (the channel exponents), and in_scale for the f16 arithmetic kinds (a power of two that puts the largest
    activation the split sees in [2^14, 2^15): with g in [-3, 3] all of them then sit in f16's normal range, conv_common.h's 22-bit window)"""
    c = case
    rng = np.random.default_rng([seed, zlib.crc32(c.name.encode()), KINDS.index(kind)])
    glim = 3 if kind in ('f16x3', 'f16') else 6
    e_c = rng.integers(-6, 7, c.Cin)
    f = rng.integers(-6, 7, c.Cout)
    g = rng.integers(-glim, glim + 1, (c.B, c.H, c.W))
    st = STORE[kind]
    rk = 1.0 / math.sqrt(c.K)
    o = {'e_c': e_c, 'f': f}
    o['x'] = _round(_vals(rng, e_c[None, :, None, None] + g[:, None]), st)
    o['w'] = _round(_vals(rng, (-e_c[None, :] + f[:, None])[:, :, None, None] + np.zeros((1, 1, c.kh, c.kw))) * rk, st)
    go = g[:, np.minimum(np.arange(c.Ho) * c.stride, c.H - 1)][:, :, np.minimum(np.arange(c.Wo) * c.stride, c.W - 1)]     # the output pixel's exponent
    o['x2'] = o['w2'] = None
    if c.Cin2:
        e2 = rng.integers(-6, 7, c.Cin2)
        g2 = rng.integers(-glim, glim + 1, (c.B, c.H2, c.W2))
        g2[:, ::c.stride2, ::c.stride2] = g                       # the pixels the second source is read at carry the first source's exponent
        o['x2'] = _round(_vals(rng, e2[None, :, None, None] + g2[:, None]), st)
        o['w2'] = _round(_vals(rng, (-e2[None, :] + f[:, None])[:, :, None, None]) * rk, st)
    sgn = (rng.integers(0, 2, c.Cout) * 2 - 1) if c.neg_scale else 1
    o['scale'] = (sgn * (0.5 + rng.random(c.Cout))).astype(np.float32) if c.scale else None
    o['shift'] = _vals(rng, f).astype(np.float32) if c.shift else None
    o['res'] = _round(_vals(rng, f[None, :, None, None] + go[:, None]), c.out_dtype(kind)) if c.residual else None
    o['ps'] = o['pb'] = None
    if c.pre:
        o['ps'] = (rng.choice([0.5, 1.0, 2.0], c.Cin) * (rng.integers(0, 2, c.Cin) * 2 - 1)).astype(np.float32)
        o['pb'] = (rng.integers(-127, 128, c.Cin) / 64.0).astype(np.float32)              # multiples of 2^-6 inside (-2, 2)
    o['in_scale'] = None
    if kind in ('f16x3', 'f16'):
        amax = max(float(np.abs(_activated(c, o, kind, scaled=False)).max()), float(np.abs(o['x2']).max()) if c.Cin2 else 0.0)
        o['in_scale'] = 2.0 ** (15 - _pow2_floor_exp(amax)) if amax > 0 else 1.0
    return o


def _activated(c, o, kind, scaled=True):
    """the convolution's first operand as the kernel forms it, float64 NCHW: x, or act(x ps + pb) rounded ONCE to the operand type (x ps + pb is
    exact in float64, and ps is a power of two, so fused and unfused fp32 evaluation round the same way); 'f16': rounded to f16 after in_scale"""
    a = o['x'].astype(np.float64)
    if c.pre:
        a = a * o['ps'].astype(np.float64)[None, :, None, None] + o['pb'].astype(np.float64)[None, :, None, None]
        if c.pre == 'relu':
            a = np.maximum(a, 0)
        a = _round(a.astype(np.float32), STORE[kind]).astype(np.float64)
    if kind == 'f16' and scaled:
        a = _f16_at(a, o['in_scale'])
    return a


def _f16_at(a, s):
    return _round((a * s).astype(np.float32), torch.float16).astype(np.float64) / s


def weight_rows(c, o):
    """[Cout, kh kw Cin (+ Cin2)] in the kernels' K order (tap-major, channels innermost; the second source's columns appended)"""
    rows = o['w'].transpose(0, 2, 3, 1).reshape(c.Cout, -1)
    return np.concatenate([rows, o['w2'].reshape(c.Cout, -1)], 1) if c.Cin2 else rows


def _operands64(c, o, kind):
    a, w = _activated(c, o, kind), o['w'].astype(np.float64)
    a2 = o['x2'].astype(np.float64) if c.Cin2 else None
    w2 = o['w2'].astype(np.float64) if c.Cin2 else None
    if kind == 'f16':
        # pack_f16x3_weights: every row times the power of two that puts its largest |w| in [2^12, 2^13), rounded to f16 (the hi part)
        amax = np.abs(weight_rows(c, o)).max(1)
        p = np.exp2(13 - np.frexp(np.where(amax > 0, amax, 1.0))[1])[:, None, None, None]
        w = _round((w * p).astype(np.float32), torch.float16).astype(np.float64) / p
        if c.Cin2:
            w2 = _round((w2 * p).astype(np.float32), torch.float16).astype(np.float64) / p
            a2 = _f16_at(a2, o['in_scale'])
    return a, w, a2, w2


def _conv(a, w, stride, pad):
    return torch.nn.functional.conv2d(torch.from_numpy(a), torch.from_numpy(w), stride=stride, padding=pad).numpy()


def reference(case, o, kind):
    """-> (ref, S), float64 [B, Cout, Ho, Wo]: the exact operation on the operands as stored -- pre-activation with its re-rounding, second
    source, scale, shift, residual, ReLU -- and S = |scale| conv(|a|, |w|) + |shift| + |residual|, the size every rounding error scales with"""
    c = case
    a, w, a2, w2 = _operands64(c, o, kind)
    ref, S = _conv(a, w, c.stride, c.pad), _conv(np.abs(a), np.abs(w), c.stride, c.pad)
    if c.Cin2:
        ref = ref + _conv(a2, w2, c.stride2, 0)
        S = S + _conv(np.abs(a2), np.abs(w2), c.stride2, 0)
    if c.scale:
        sc = o['scale'].astype(np.float64)[None, :, None, None]
        ref, S = ref * sc, S * np.abs(sc)
    if c.shift:
        sh = o['shift'].astype(np.float64)[None, :, None, None]
        ref, S = ref + sh, S + np.abs(sh)
    if c.residual:
        ref, S = ref + o['res'], S + np.abs(o['res'])
    if c.relu:
        ref = np.maximum(ref, 0)
    return ref, S


def float32_result(case, o, kind, conv=None):
    """the same operation in plain float32 on the CPU (torch conv2d, float32 epilogue in the kernels' order), NOT rounded to the output type:
    what the CPU tests hold against the bound, and the clean result the defects of test_conv_cases_ref.py are applied to"""
    c = case
    a, w, a2, w2 = (None if t is None else t.astype(np.float32) for t in _operands64(c, o, kind))
    v = _conv(a, w, c.stride, c.pad) if conv is None else conv(a, w, a2, w2)
    if c.Cin2 and conv is None:
        v = v + _conv(a2, w2, c.stride2, 0)
    if c.scale:
        v = v * o['scale'][None, :, None, None]
    if c.shift:
        v = v + o['shift'][None, :, None, None]
    if c.residual:
        v = v + o['res']
    if c.relu:
        v = np.maximum(v, 0)
    return v.astype(np.float32)


def to_buffer(case, kind, v, fill=3.0):
    """a float NCHW result -> the NHWC output buffer [B, Ho, Wo, out_cs] in the output type (f16 saturating like the kernels' stores), `fill` in
    the canary channels"""
    c, dt = case, case.out_dtype(kind)
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(v, (0, 2, 3, 1)))).float()
    if dt == torch.float16:
        t = t.clamp(-65504.0, 65504.0)
    buf = torch.full((c.B, c.Ho, c.Wo, c.out_cs), fill, dtype=dt)
    buf[..., c.out_coff:c.out_coff + c.Cout] = t.to(dt)
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------- check
F16_MAX = 65504.0


def c_eff(case, kind, c=None):
    """c(kind), capped so that acc never exceeds what the arithmetic guarantees: (K + 2) 2^-24 S for exact fp32 products summed in fp32 (the
    exact-fp32, 16-bit and f16 kinds), 2^-20 S for f16x3 (conv_common.h's ~2^-22 per product, times the project's margin of 4)"""
    c = C[kind] if c is None else c
    K = case.K
    return min(c, 16.0 / math.sqrt(K)) if kind == 'f16x3' else min(c, (K + 2) / math.sqrt(K))


def _half_ulp(v, dt):
    v = np.maximum(np.abs(v), 1e-300)
    e = np.floor(np.log2(v))
    if dt == torch.bfloat16:
        return 0.5 * np.exp2(np.maximum(e, -126) - 7)
    return 0.5 * np.exp2(np.maximum(e, -14) - 10)


def bound(ref, S, case, kind, c=None):
    """-> (unit, acc, tol): unit = sqrt(K) 2^-24 S, acc = c unit, tol = acc + half an ulp of the output type at |ref| + acc (0 for fp32)"""
    unit = math.sqrt(case.K) * 2.0 ** -24 * S
    acc = c_eff(case, kind, c) * unit
    dt = case.out_dtype(kind)
    rt = 0.0 if dt == torch.float32 else _half_ulp(np.minimum(np.abs(ref) + acc, F16_MAX) if dt == torch.float16 else np.abs(ref) + acc, dt)
    return unit, acc, acc + rt


def check(got, ref, S, case, kind, c=None, fill=3.0, enforce=True):
    """got: the whole NHWC output buffer (torch, on the CPU, in the output type) a kernel wrote over `fill`.  Every element must lie within
    acc + round_T(ref, acc) of ref; an f16 output must be +-65504 where ref lies beyond it by more than acc; canary channels keep their bits.
    -> the largest (|got - ref| - round_T) / (sqrt(K) 2^-24 S): the accumulation error in units of the bound at c = 1.  enforce=False: measure only"""
    cs, dt = case, case.out_dtype(kind)
    assert tuple(got.shape) == (cs.B, cs.Ho, cs.Wo, cs.out_cs) and got.dtype == dt, (tuple(got.shape), got.dtype)
    can = torch.full((1,), fill, dtype=dt)
    left, right = got[..., :cs.out_coff], got[..., cs.out_coff + cs.Cout:]
    iv = {torch.float32: torch.int32}.get(dt, torch.int16)
    if enforce:
        for name, part in (('below', left), ('above', right)):
            assert bool((part.contiguous().view(iv) == can.view(iv)).all()), '%s: canary channels %s the slice were written' % (cs.name, name)
    g = got[..., cs.out_coff:cs.out_coff + cs.Cout].double().numpy().transpose(0, 3, 1, 2)
    unit, acc, tol = bound(ref, S, cs, kind, c)
    refc = np.clip(ref, -F16_MAX, F16_MAX) if dt == torch.float16 else ref
    d = np.abs(g - refc)
    bad = ~(d <= tol)                                            # (NaN fails)
    if dt == torch.float16:
        sat = np.abs(ref) - acc > F16_MAX
        bad |= sat & (g != np.sign(ref) * F16_MAX)
    excess = np.maximum(d - (tol - acc), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(unit > 0, excess / unit, np.where(excess > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(g), ratio, np.inf)
    if enforce and bad.any():
        idx = np.argwhere(bad)
        worst = idx[np.argmax(np.where(bad, np.where(np.isfinite(ratio), ratio, 1e300), -1.0)[bad])]
        b, n, y, x = (int(i) for i in worst)
        raise AssertionError('%s [%s]: %d of %d elements outside the bound; worst at (b %d, y %d, x %d, n %d): got %r, ref %r, allowed %.3e, '
                             'accumulation part %.3e (%.2f x the c = 1 unit)' % (cs.name, kind, len(idx), bad.size, b, y, x, n, float(g[b, n, y, x]),
                                                                                 float(ref[b, n, y, x]), float(np.broadcast_to(tol, bad.shape)[b, n, y, x]),
                                                                                 float(np.broadcast_to(acc, bad.shape)[b, n, y, x]), float(ratio[b, n, y, x])))
    return float(ratio.max())
