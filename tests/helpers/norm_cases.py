"""Edge cases of the fp32 training operators of csrc/train_ops.hip (the BatchNorm family, LayerNorm, attention, GELU, column sums): case lists,
operands with per-channel scale structure, float64 references and a per-element check.  CPU only (numpy + torch CPU + scipy):
tests/test_norm_cases_ref.py proves the pieces here, tests/test_gpu_norm_sweep.py points the kernels at them.

check(got, ref, S, c)      every element: |got - ref| <= c 2^-24 S + 2^-140 (512 of fp32's smallest spacings: sums of products that underflow).  S is the element's first-order error
                           scale: what one unit roundoff (2^-24) in every operation the element passes through can move it by, written with
                           absolute values.  Each S has three parts -- the output's own rounding, the error of the mean it uses, the error of the
                           variance / normaliser it uses.

BatchNorm over x [R, C] (per channel; mbar = mean |x|, xh = (x - mean) rstd, u = 2^-24):
  mean          S = mbar                       a sum of R terms moves by at most (R - 1) u sum|x|; the division adds u |mean| <= u mbar
  var (biased)  S = var + (2 / R) sum_k n_k |m_k - m_parent| (mbar_k + mbar_parent) + u C_MEAN^2 mbar^2
                                               own: the squared deviations and their sum.  A one-chunk two-pass variance has no first-order term
                                               in the error of its mean (sum (x - mean) = 0); the documented chunk pooling
                                               sum_k [M2_k + n_k (m_k - m)^2] has one per level: 2 n_k |m_k - m| dm_k, dm_k <= c u mbar_k.  The
                                               last term is the second-order n dm^2 with dm = C_MEAN u mbar: at mean / sigma = 10^5 it is
                                               larger than the first-order ones (a ONE-pass variance errs by ~u mbar^2: 2^24 / C_MEAN^2 times it)
  rstd          S = rstd (1 + S_var / (2 (var + eps)))
  running_*     S = |(1 - m) old| + m S_stat + |new|            (S_var times R / (R - 1) for the unbiased variance)
  pre_scale     k = w rstd: S = |w| S_rstd + |k| ;  pre_shift = b - mean k: S = |b| + |mean| (|w| S_rstd + |k|) + |k| mbar + |pre_shift|
  y             S = |w| rstd mbar + 2 |w| |xh| + |y| + |b| (+ |residual|)        error of the mean | of rstd and of x - mean | own
                (statistics given as operands -- frozen, SyncBN's normalisation: no mean term)
  backward      takes the forward's saved mean / rstd AS OPERANDS (the kernels do): xh is then exact to 2 u.  g = gy under the ReLU mask.
  gb            S = sum |g| ;  gw: S = 2 sum |g xh|
  gx            = w rstd (g - m1 - xh m2): S = |w| rstd (|g| + |m1| + S_gb / R + |xh| (2 |m2| + S_gw / R)) + |gx|
  ReLU          the mask is the float64 one, except on the UNDECIDED BAND |pre-activation| <= its own bound, where the reference takes the
                mask the kernel's forward produced; off the band the kernel's mask must equal the float64 mask (relu_resolve).
LayerNorm: the same forms per row (sums over the C columns; gw / gb are sums over the R rows).
Attention (per sample and head; s = scale q.k, SL = scale sum |q| |k|, p = softmax(s)):
  probs         S = p (SL_ij + sum_l p_il SL_il + |s_ij| + |s_ij - max_i| + 4)      own logit | the normaliser | scaling, max subtraction, exp, sum, division
  out           S = sum_j (S_p_ij + p_ij) |v_jd|
  backward      takes the saved probs as operands.  gv: S = sum_i |P_ij go_id| ;  gP = go.v: S_gP = sum |go| |v| ;  dot_i = sum_j gP P:
                S_dot = sum_j (S_gP + |gP|) P ;  gS = scale P (gP - dot): S_gS = scale P (S_gP + S_dot + 2 |gP - dot|) + |gS| ;
                gq = gS k: S = sum_j (S_gS_ij + |gS_ij|) |k_jd| ;  gk = gS^T q likewise
GELU            y = x (1 + erf(x / sqrt 2)) / 2: S = |x| (1 + |erf|) / 2 -- the 1 + erf cancellation at negative x is inherent to the formula and S
                carries it ;  gx = gy (cdf + x pdf): S = |gy| ((1 + |erf|) / 2 + |x| pdf (2 + x^2)) + |gx|      (x^2: the exponent's rounding)
column sums     S = sum |x| (+ |old| + |new| when accumulating)

The constants c (C below), one per output kind, are NOT measured on the kernels: each is 4 x the largest |ref32 - ref64| / (2^-24 S) over the whole
case list (RATIOS below; tests/test_norm_cases_ref.py re-measures them), ref32 the worse of (a) torch's own CPU float32 operator and (b) a numpy
float32 evaluation in the order the kernels document (two passes, 256-row chunks pooled with the n_k d^2 term).  4 is the project's margin for a
different, equally valid summation order (tests/helpers/conv_cases.py).  c_eff caps c at the serial bound: the longest chain of additions an
element passes through (+ 4 single roundings)."""
import collections
import zlib

import numpy as np
import torch
from scipy.special import erf

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -140
EPS, MOMENTUM = 1e-5, 0.1
BN_SMALL_R, BN_CHUNK, COARSEN_PER = 512, 256, 32
PAIRS = ((0.0, 1.0), (1e3, 1.0), (1e3, 1e-2), (0.0, 1e-4), (-50.0, 30.0), (7.0, 0.0), (3e4, 1.0), (0.0, 1e3))      # (mean, sigma) per channel / row
KAPPA_RELU = 2.0 ** 10            # ReLU variants use only channels with max|x| rstd <= 2^10 (others are redrawn as (0, 1))
TORCH_THREADS = 8                 # reference (a) is measured with torch on 8 threads (its row reductions split by the thread count)
BAND_CAP = 0.005                  # the undecided band may hold at most 0.5 % of a case's elements
BN_CLASSES = ('small', 'mid', 'chunk_vec', 'chunk_scalar', 'strided', 'split', 'partials', 'sync', 'frozen')
BN_VARIANTS = ('plain', 'relu', 'relu_res', 'no_gx', 'no_wb')
BN_CHANNELS = (1, 3, 4, 6, 8, 12, 16, 20, 36, 60, 64, 68, 132, 260)
MID_R = (16, 17, 63, 64, 65, 192, 193, 256, 257, 449, 511, 512)
CHUNK_R = tuple(512 + d for d in (1, 16, 17, 49, 65, 255, 256)) + tuple(256 * k + 5 for k in (15, 16, 17, 32))
LN_C = (1, 2, 63, 64, 65, 128, 129, 255, 256)
LN_R = (1, 3, 4, 5, 15, 16, 17, 48, 49, 64, 65, 113)
ATT_T, ATT_H, ATT_B, ATT_D = (1, 2, 21, 42, 63, 64), (1, 4, 5), (1, 3), 32
ATT_KINDS = ('normal', 'large', 'onehot', 'uniform', 'qzero')
GELU_VALUES = (0.0, 1e-40, 1e-30, 1e-4, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 5.5, 6.0, 8.0, 10.0, 13.0, 38.0, 1e4, 1e19)
COLSUM_R = (1, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097)
COLSUM_N = (1, 4, 36, 60, 64, 68)

# measured |ref32 - ref64| / (2^-24 S), the worse of the two float32 references over the whole list (test_reference_error_... prints them)
RATIOS = {'bn_mean': 15.7, 'bn_var': 6.14, 'bn_rstd': 4.92, 'bn_running': 8.05, 'bn_pre': 2.56, 'bn_y': 15.7, 'bn_gx': 2.63, 'bn_gw': 1.87, 'bn_gb': 3.41,
          'ln_mean': 5.81, 'ln_rstd': 46.3, 'ln_y': 2.63, 'ln_gx': 1.46e5, 'ln_gw': 1.22e6, 'ln_gb': 5.56,
          'att_probs': 2.37, 'att_out': 1.48, 'att_gq': 0.938, 'att_gk': 1.30, 'att_gv': 7.20, 'gelu_y': 5.22, 'gelu_gx': 3.78, 'colsum': 16.8}
# (a) torch on TORCH_THREADS threads | (b) numpy in kernel order, where they differ much: bn_mean 10.1 | 15.7 (a serial sum of 512 rows near 10^3;
# on ONE thread torch sums up to 8197 rows serially and is at 55.3, which would put 0.5 % of a ReLU case into the undecided band), bn_y 7.47 | 15.7,
# bn_rstd 2.85 | 4.92, bn_running 4.97 | 8.05, ln_rstd 46.2 | 1.86, ln_gx 1.45e5 | 1.00, ln_gw 1.21e6 | 3.08 (torch's CPU LayerNorm takes one-pass
# moments and an expanded backward: at mean / sigma >= 10^3 its gradients are beyond any first-order scale, so for ln_gx / ln_gw / ln_rstd the
# serial cap of c_eff is what binds), gelu_y 5.22 | 1.96, gelu_gx 3.78 | 1.32; bn_var, bn_pre (SyncBN, the split entry points) and colsum
# (16.8: a serial sum of 511 rows) have no torch operator
C_MEAN = 16.0                                                         # the mean's constant inside S_var's second-order term (>= reference (b)'s own mean error, 15.7)
C = {k: 4.0 * v for k, v in RATIOS.items()}


NO_CHAIN = 1 << 30                 # GELU: no chain of additions (erf and exp are library evaluations): uncapped


def c_eff(kind, chain):
    """c of one output kind, capped at the serial bound of a case: `chain` additions + 4 single roundings"""
    return min(C[kind], chain + 4.0)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def ratio(got, ref, S):
    """max (|got - ref| - 2^-140) / (2^-24 S) over the elements (0 where that is <= 0; inf for a non-finite got)"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float('inf')
    e = np.maximum(np.abs(got - ref) - TINY, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e > 0, e / (U * S), 0.0)
    return float(r.max())


def check(got, ref, S, c, what=''):
    """every element |got - ref| <= c 2^-24 S + 2^-140; -> the largest ratio (in units of 2^-24 S)"""
    r = ratio(got, ref, S)
    if not r <= c:
        got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
        bad = ~(np.abs(got - ref) <= c * U * S + TINY)
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError('%s: %d of %d elements outside c 2^-24 S (c = %.3g, worst ratio %.4g); first at %s: got %.9g, ref %.9g, S %.4g'
                             % (what, int(bad.sum()), bad.size, c, r, i, got[i], ref[i], S[i]))
    return r


# ===================================================================================================================== BatchNorm: the cases
BnCase = collections.namedtuple('BnCase', 'name cls api R C ld mis chunk_rows cap splits')


def _bn(cls, api, R, C, ld=0, mis=False, chunk_rows=0, cap=0, splits=(), tag=''):
    ld = ld or C
    name = '%s-%s-R%d-C%d' % (cls, api, R, C) + ('-ld%d' % ld if ld != C else '') + ('-mis' if mis else '') + tag
    return BnCase(name, cls, api, R, C, ld, mis, chunk_rows, cap, tuple(splits))


SYNC_SPLITS = {1: (600,), 2: (1, 599), 3: (300, 1, 523), 8: (1, 17, 256, 257, 300, 513, 64, 5)}


def bn_cases(cls=None):
    L = []
    for R in (1, 2, 15):
        L += [_bn('small', 'train', R, C) for C in (1, 3, 4, 8, 20, 64, 260)]
    L += [_bn('small', 'train', R, C) for R, C in ((16, 3), (64, 6), (100, 1), (257, 3), (512, 6), (193, 1))]
    L += [_bn('mid', 'train', R, C) for R in MID_R for C in (4, 8, 20, 36, 68, 132)]
    L += [_bn('chunk_vec', 'train', R, C) for R in CHUNK_R for C in (4, 60, 64, 68, 132)]
    L += [_bn('chunk_scalar', 'train', R, C) for R in CHUNK_R for C in (3, 6)]
    L += [_bn('chunk_scalar', 'train', R, 8, mis=True) for R in (513, 577, 768, 4101)]
    for R, C in ((15, 8), (193, 20), (577, 68), (4101, 60)):
        L += [_bn('strided', 'train', R, C, ld=C + 4), _bn('strided', 'train', R, C, ld=C + 1)]
    L += [_bn('split', 'split', R, C) for R, C in ((529, 64), (577, 132), (4101, 68))]
    for rows, Cs in ((8, (4, 20, 68)), (64, (4, 20, 68))):
        for chunks, short in ((255, 0), (256, 0), (257, 0), (257, rows // 2 + 1)):
            for C in Cs:
                R = chunks * rows - short
                L.append(_bn('partials', 'partials', R, C, chunk_rows=rows, cap=chunks + (chunks + COARSEN_PER - 1) // COARSEN_PER))
    L.append(_bn('partials', 'partials', 257 * 8, 20, chunk_rows=8, cap=257, tag='-flat'))
    for W, sp in sorted(SYNC_SPLITS.items()):
        L += [_bn('sync', 'sync', sum(sp), C, splits=sp, tag='-W%d' % W) for C in (4, 20, 68)]
    L += [_bn('frozen', 'frozen', R, C) for R, C in ((193, 20), (577, 68), (577, 6))]
    return [c for c in L if cls is None or c.cls == cls]


def bn_vec4(C, ld, aligned):
    """train_ops.hip's bn_vec4: 16-byte loads need C % 4 == 0, ld % 4 == 0 and 16-byte aligned pointers"""
    return C % 4 == 0 and ld % 4 == 0 and aligned


def bn_path(case):
    """the dispatch of dir_bn_train_forward / _backward restated: 'small' (one thread per channel), 'mid' (cooperative, 16 <= R <= 512, vector),
    'chunk_vec' (R > 512, vector), 'chunk_scalar' (R > 512, scalar)"""
    vec = bn_vec4(case.C, case.ld, not case.mis)
    if case.R <= BN_SMALL_R:
        return 'mid' if case.R >= 16 and case.C >= 4 and vec else 'small'
    return 'chunk_vec' if vec else 'chunk_scalar'


def bn_expected_kernels(case, variant):
    """(forward launches, backward launches) by the names at the DIR_LAUNCH sites, for the api of the case"""
    relu, gx = variant in ('relu', 'relu_res'), variant != 'no_gx'
    p = bn_path(case)
    bwd_vec = ['bn_bwd_partial4_kernel', 'bn_bwd_combine_kernel'] + (['bn_apply_bwd4_kernel'] if gx else [])
    if case.api == 'train':
        fwd = {'small': ['bn_train_fwd_kernel'], 'mid': ['bn_mid_fwd_kernel'],
               'chunk_vec': ['bn_stats4_kernel', 'bn_stats_combine_kernel', 'bn_apply_fwd4_kernel'],
               'chunk_scalar': ['bn_partial_kernel', 'bn_colsum_chunks_kernel', 'bn_partial_kernel', 'bn_stats_finalize_kernel', 'bn_apply_fwd_kernel']}[p]
        bwd = {'small': ['bn_train_bwd_kernel'], 'mid': ['bn_mid_bwd_kernel'], 'chunk_vec': bwd_vec,
               'chunk_scalar': ['bn_partial_kernel', 'bn_bwd_combine_kernel'] + (['bn_apply_bwd_kernel'] if gx else [])}[p]
        return fwd, bwd
    if case.api == 'split':
        return ['bn_stats4_kernel', 'bn_stats_combine_pre_kernel', 'bn_apply_fwd4_kernel'], bwd_vec
    if case.api == 'partials':
        chunks = (case.R + case.chunk_rows - 1) // case.chunk_rows
        two = chunks > 256 and case.cap >= chunks + (chunks + COARSEN_PER - 1) // COARSEN_PER
        return (['bn_partials_coarsen_kernel'] if two else []) + ['bn_stats_combine_pre_kernel', 'bn_apply_fwd4_kernel'], bwd_vec[1:]
    if case.api == 'sync':
        W = len(case.splits)
        return (['bn_stats4_kernel', 'bn_stats_local_kernel'] * W + ['bn_sync_combine_kernel'] + ['bn_frozen_stats_kernel', 'bn_apply_fwd4_kernel'] * W,
                ['bn_bwd_partial4_kernel', 'bn_bwd_sums_kernel'] * W + (['bn_apply_bwd4_kernel'] * W if gx else []))
    vec = bn_vec4(case.C, case.ld, not case.mis)                      # frozen
    return (['bn_frozen_stats_kernel', 'bn_apply_fwd4_kernel' if vec else 'bn_apply_fwd_kernel'],
            ['bn_bwd_partial4_kernel' if vec else 'bn_partial_kernel', 'bn_bwd_combine_kernel'] +
            (['zero_f32_kernel', 'bn_apply_bwd4_kernel' if vec else 'bn_apply_bwd_kernel'] if gx else []))


# the kernels each class is there to reach: each must serve at least three of the class's cases (where the variant launches it at all)
BN_EXPECTED = {'small': ('bn_train_fwd_kernel', 'bn_train_bwd_kernel'), 'mid': ('bn_mid_fwd_kernel', 'bn_mid_bwd_kernel'),
               'chunk_vec': ('bn_stats4_kernel', 'bn_stats_combine_kernel', 'bn_apply_fwd4_kernel', 'bn_bwd_partial4_kernel', 'bn_bwd_combine_kernel',
                             'bn_apply_bwd4_kernel'),
               'chunk_scalar': ('bn_partial_kernel', 'bn_colsum_chunks_kernel', 'bn_stats_finalize_kernel', 'bn_apply_fwd_kernel', 'bn_apply_bwd_kernel'),
               'strided': (), 'split': ('bn_stats_combine_pre_kernel',), 'partials': ('bn_partials_coarsen_kernel', 'bn_stats_combine_pre_kernel'),
               'sync': ('bn_stats_local_kernel', 'bn_sync_combine_kernel', 'bn_bwd_sums_kernel'), 'frozen': ('bn_frozen_stats_kernel',)}


def bn_class_kernels(cls, variant):
    """BN_EXPECTED[cls] without what the variant does not launch (no backward under relu_res, no g x kernels under no_gx)"""
    out = []
    for k in BN_EXPECTED[cls]:
        n = sum(k in fb[0] + (fb[1] if variant != 'relu_res' else []) for fb in (bn_expected_kernels(c, variant) for c in bn_cases(cls)))
        if n:
            out.append(k)
    return out


def _starts(R, rows):
    return np.arange(0, R, rows)


def bn_levels(case):
    """the pooling levels the kernels document, fine -> coarse, each a sorted array of chunk starts ([]: one two-pass over all rows)"""
    if case.api in ('train', 'split'):
        return [_starts(case.R, BN_CHUNK)] if case.R > BN_SMALL_R else []
    if case.api == 'partials':
        chunks = (case.R + case.chunk_rows - 1) // case.chunk_rows
        lv = [_starts(case.R, case.chunk_rows)]
        if chunks > 256 and case.cap >= chunks + (chunks + COARSEN_PER - 1) // COARSEN_PER:
            lv.append(_starts(case.R, case.chunk_rows * COARSEN_PER))
        return lv
    if case.api == 'sync':
        rank0 = np.cumsum((0,) + case.splits[:-1])
        fine = np.concatenate([r0 + _starts(n, BN_CHUNK) for r0, n in zip(rank0, case.splits)])
        return [fine, rank0]
    return []


# ===================================================================================================================== BatchNorm: operands
def bn_make(case, variant):
    """x = mu_c + sigma_c N(0, 1) with (mu_c, sigma_c) cycling through PAIRS, one (0, 1) channel + 100 on the first half of the rows; w ~ N(0, 1),
    b ~ N(0, 0.5), gy ~ N(0, 1) 2^e_c (e_c in [-8, 8]), residual ~ N(0, 1); SyncBN: rank r's rows + 100 sigma_c (r % 3)"""
    rng = _rng(case.name)
    R, Cn = case.R, case.C
    mu = np.array([PAIRS[c % 8][0] for c in range(Cn)])
    sg = np.array([PAIRS[c % 8][1] for c in range(Cn)])
    x = mu + sg * rng.normal(0, 1, (R, Cn))
    oc = 8 if Cn > 8 else 0
    x[:(R + 1) // 2, oc] += 100.0
    if case.api == 'sync':
        r0 = 0
        for r, n in enumerate(case.splits):
            x[r0:r0 + n] += 100.0 * sg * (r % 3)
            r0 += n
    x = x.astype(F)
    w, b = rng.normal(0, 1, Cn).astype(F), rng.normal(0, 0.5, Cn).astype(F)
    e = (5 * np.arange(Cn)) % 17 - 8
    gy = (rng.normal(0, 1, (R, Cn)) * 2.0 ** e).astype(F)
    res = rng.normal(0, 1, (R, Cn)).astype(F)
    rm0, rv0 = rng.normal(0, 1, Cn).astype(F), rng.uniform(0.5, 2, Cn).astype(F)
    relu = variant in ('relu', 'relu_res')
    if relu and case.api != 'frozen':
        x64 = x.astype(np.float64)
        kap = np.abs(x64).max(0) / np.sqrt(x64.var(0) + EPS)
        r2 = _rng(case.name + '/relu')
        for c in np.nonzero(kap > KAPPA_RELU)[0]:
            x[:, c] = r2.normal(0, 1, R).astype(F)
    if case.api == 'frozen':                                          # statistics near the batch's, running_var with 0, 1e-12 and 1e6
        x64 = x.astype(np.float64)
        rm0 = (x64.mean(0) + 0.1 * x64.std(0) * rng.normal(0, 1, Cn)).astype(F)
        rv0 = (x64.var(0) * rng.uniform(0.5, 2, Cn)).astype(F)
        for i, v in enumerate((0.0, 1e-12, 1e6)):
            rv0[i % Cn] = v
    o = dict(x=x, w=w, b=b, gy=gy, res=res if variant == 'relu_res' else None, rm0=rm0, rv0=rv0, relu=relu, need_gx=variant != 'no_gx')
    if variant == 'no_wb':
        o['w'] = o['b'] = None
    if case.api == 'partials':
        o['p1'], o['p2'] = bn_partials32(x, case.chunk_rows)
    return o


def bn_partials32(x, rows):
    """chunk partials by their documented meaning, in float32: column sum | sum of squared deviations from the chunk's own mean"""
    p1, p2 = [], []
    for a in range(0, x.shape[0], rows):
        blk = x[a:a + rows]
        s = np.add.reduce(blk, 0, dtype=F)
        d = blk - s / F(blk.shape[0])
        p1.append(s)
        p2.append(np.add.reduce(d * d, 0, dtype=F))
    return np.stack(p1), np.stack(p2)


# ===================================================================================================================== BatchNorm: float64 references
def _level_stats(x64, levels):
    """per level: (n_k [K], m_k [K, C], mbar_k [K, C], parent index [K]); the last level's parent is the whole batch"""
    R = x64.shape[0]
    ax = np.abs(x64)
    out = []
    for i, st in enumerate(levels):
        n = np.diff(np.append(st, R)).astype(np.float64)
        m, mb = np.add.reduceat(x64, st, axis=0) / n[:, None], np.add.reduceat(ax, st, axis=0) / n[:, None]
        par = np.searchsorted(levels[i + 1], st, 'right') - 1 if i + 1 < len(levels) else np.zeros(len(st), int)
        out.append((n, m, mb, par))
    return out


def bn_stats_ref(x64, levels, partials=None):
    """-> dict mean, var (biased), rstd and their S.  partials = (p1, p2) as stored: the statistics are then functions of THOSE operands"""
    R = x64.shape[0]
    if partials is None:
        mean, var, mbar = x64.mean(0), x64.var(0), np.abs(x64).mean(0)
        ls = _level_stats(x64, levels)
    else:
        p1, p2 = (a.astype(np.float64) for a in partials)
        n0 = np.diff(np.append(levels[0], R)).astype(np.float64)
        mean, mbar = p1.sum(0) / R, np.abs(p1).sum(0) / R
        var = (p2 + n0[:, None] * (p1 / n0[:, None] - mean) ** 2).sum(0) / R
        ls = []
        for i, st in enumerate(levels):                               # a coarser level's sums are sums of the stored chunk sums
            idx = np.searchsorted(st, levels[0], 'right') - 1
            n = np.bincount(idx, n0)
            s, sa = (np.stack([np.bincount(idx, a[:, c]) for c in range(a.shape[1])], 1) for a in (p1, np.abs(p1)))
            par = np.searchsorted(levels[i + 1], st, 'right') - 1 if i + 1 < len(levels) else np.zeros(len(st), int)
            ls.append((n, s / n[:, None], sa / n[:, None], par))
    first = np.zeros_like(mean)
    for i, (n, m, mb, par) in enumerate(ls):
        pm, pmb = (ls[i + 1][1][par], ls[i + 1][2][par]) if i + 1 < len(ls) else (mean[None], mbar[None])
        first += (n[:, None] * np.abs(m - pm) * (mb + pmb)).sum(0)
    S_var = var + 2.0 / R * first + U * C_MEAN ** 2 * mbar ** 2
    rstd = 1.0 / np.sqrt(var + EPS)
    return dict(mean=mean, var=var, rstd=rstd, mbar=mbar, S_mean=mbar, S_var=S_var, S_rstd=rstd * (1 + S_var / (2 * (var + EPS))), R=R)


def bn_running_ref(st, rm0, rv0):
    """R = 1 follows the kernels' stated rule: running_var takes the biased variance"""
    R, m = st['R'], MOMENTUM
    k = R / (R - 1.0) if R > 1 else 1.0
    rm = (1 - m) * rm0.astype(np.float64) + m * st['mean']
    rv = (1 - m) * rv0.astype(np.float64) + m * st['var'] * k
    return ((rm, np.abs((1 - m) * rm0) + m * st['S_mean'] + np.abs(rm)), (rv, np.abs((1 - m) * rv0) + m * st['S_var'] * k + np.abs(rv)))


def bn_pre_ref(st, w, b):
    w64 = 1.0 if w is None else w.astype(np.float64)
    b64 = 0.0 if b is None else b.astype(np.float64)
    k = w64 * st['rstd']
    Sk = np.abs(w64) * st['S_rstd'] + np.abs(k)
    sh = b64 - st['mean'] * k
    return (k, Sk), (sh, np.abs(b64) + np.abs(st['mean']) * Sk + np.abs(k) * st['S_mean'] + np.abs(sh))


def relu_resolve(pre, S, c, got):
    """the ReLU of a float64 pre-activation against the kernel's output: -> (reference, mask used, band, kernel mask wrong off the band)"""
    band = np.abs(pre) <= c * U * S + TINY
    m64, mk = pre > 0, np.asarray(got) > 0
    mask = np.where(band, mk, m64)
    return np.where(mask, pre, 0.0), mask, band, (mk != m64) & ~band


def bn_y_ref(x64, w, b, mean, rstd, S_mean, res=None):
    """pre-activation and its S (S_mean = 0 where the statistics are operands)"""
    w64 = np.ones(x64.shape[1]) if w is None else w.astype(np.float64)
    b64 = np.zeros(x64.shape[1]) if b is None else b.astype(np.float64)
    xh = (x64 - mean) * rstd
    y = xh * w64 + b64
    S = np.abs(w64) * rstd * S_mean + 2 * np.abs(w64 * xh) + np.abs(y) + np.abs(b64)
    if res is not None:
        y = y + res.astype(np.float64)
        S = S + np.abs(res) + np.abs(y)
    return y, S


def bn_bwd_ref(gy, x64, w, mean, rstd, mask, n_pool=None, sums=None, frozen=False):
    """analytic backward with the saved statistics as operands: -> dict gb, gw, gx -> (ref, S).  n_pool / sums = (s1, s2, S1, S2): SyncBN's pooled
    row count and sums (gb / gw stay this rank's); frozen: gx = gy w rstd"""
    R, Cn = x64.shape
    w64 = np.ones(Cn) if w is None else w.astype(np.float64)
    g = np.where(mask, gy.astype(np.float64), 0.0) if mask is not None else gy.astype(np.float64)
    xh = (x64 - mean) * rstd
    s1, s2, S1, S2 = g.sum(0), (g * xh).sum(0), np.abs(g).sum(0), 2 * np.abs(g * xh).sum(0)
    out = dict(gb=(s1, S1), gw=(s2, S2), sums=(s1, s2, S1, S2))
    if frozen:
        gx = w64 * rstd * g
        out['gx'] = (gx, 3 * np.abs(gx))
        return out
    p1, p2, P1, P2 = sums if sums is not None else (s1, s2, S1, S2)
    n = float(n_pool or R)
    m1, m2 = p1 / n, p2 / n
    gx = w64 * rstd * (g - m1 - xh * m2)
    out['gx'] = (gx, np.abs(w64) * rstd * (np.abs(g) + np.abs(m1) + P1 / n + np.abs(xh) * (2 * np.abs(m2) + P2 / n)) + np.abs(gx))
    return out


# ===================================================================================================================== BatchNorm: float32 stand-ins
def bn_pool32(p1, p2, n, starts, coarser, R, drop=(), last_full=False, level=0):
    """the documented pooling in float32: sums in chunk order, var = sum_k [M2_k + n_k (m_k - m)^2] / R.  Defects: drop = levels whose n_k d^2
    term is left out; last_full = the short last chunk counted as a full one"""
    while True:
        idx = np.searchsorted(coarser[0], starts, 'right') - 1 if coarser else np.zeros(len(starts), int)
        q1, q2, nn = [], [], []
        for g in range(int(idx.max()) + 1):
            sel = idx == g
            t = np.add.reduce(p1[sel], 0, dtype=F)
            ng = F(n[sel].sum())
            nk = n[sel].astype(F)[:, None].copy()
            if last_full and level == 0 and g == int(idx.max()):
                nk[-1] = n[0]
            d = p1[sel] / nk - t / ng
            q = np.add.reduce((nk * d * d if level not in drop else F(0)) + p2[sel], 0, dtype=F)
            q1.append(t), q2.append(q), nn.append(ng)
        if not coarser:
            return q1[0] / F(R), q2[0] / F(R), q2[0]
        p1, p2, n, starts, coarser, level = np.stack(q1), np.stack(q2), np.array(nn, F), coarser[0], coarser[1:], level + 1


def bn_stats32(x, levels, partials=None, one_pass=False, drop=(), last_full=False):
    """-> (mean, biased var, M2) in float32, in the kernels' documented order"""
    R = x.shape[0]
    if one_pass:
        mean = np.add.reduce(x, 0, dtype=F) / F(R)
        var = np.add.reduce(x * x, 0, dtype=F) / F(R) - mean * mean
        return mean, np.maximum(var, F(0)), var * F(R)
    st = levels[0] if levels else np.array([0])
    if partials is None:
        b = np.append(st, R)
        parts = [bn_partials32(x[a:e], e - a) for a, e in zip(b[:-1], b[1:])]
        p1, p2 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        p1, p2 = partials
    return bn_pool32(p1, p2, np.diff(np.append(st, R)).astype(F), st, list(levels[1:]), R, drop, last_full)


def bn_fwd32(o, case, mean, var, biased_running=False, mask_no_bias=False):
    """everything dir_bn_train_forward writes, in float32 from float32 statistics"""
    x, w, b, R = o['x'], o['w'], o['b'], case.R
    rs = (F(1) / np.sqrt(var + F(EPS))).astype(F)
    w_, b_ = (np.ones(case.C, F) if w is None else w), (np.zeros(case.C, F) if b is None else b)
    y = (x - mean) * rs * w_ + b_
    if o['res'] is not None:
        y = y + o['res']
    if o['relu']:
        y = np.where((x - mean) * rs * w_ > 0, y, F(0)) if mask_no_bias else np.maximum(y, F(0))
    unb = var * F(R) / F(R - 1) if R > 1 and not biased_running else var
    m = F(MOMENTUM)
    k = w_ * rs
    return dict(y=y.astype(F), mean=mean, rstd=rs, running_mean=(F(1) - m) * o['rm0'] + m * mean, running_var=(F(1) - m) * o['rv0'] + m * unb,
                pre_scale=k, pre_shift=b_ - mean * k)


def bn_bwd32(o, case, mean, rs, mask, n_div=None, frozen=False):
    x, w, gy = o['x'], o['w'], o['gy']
    w_ = np.ones(case.C, F) if w is None else w
    g = np.where(mask, gy, F(0)) if mask is not None else gy
    xh = (x - mean) * rs
    s1, s2 = np.add.reduce(g, 0, dtype=F), np.add.reduce(g * xh, 0, dtype=F)
    n = F(n_div or case.R)
    gx = w_ * rs * g if frozen else w_ * rs * (g - s1 / n - xh * (s2 / n))
    return dict(gb=s1, gw=s2, gx=gx.astype(F))


def bn_torch32(o, case):
    """torch's own CPU float32 BatchNorm (+ residual, ReLU) and its autograd; R > 1 (torch refuses one value per channel)"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    x = t(o['x']).requires_grad_(True)
    w, b = (None if o['w'] is None else t(o['w']).requires_grad_(True)), (None if o['b'] is None else t(o['b']).requires_grad_(True))
    rm, rv = t(o['rm0'].copy()), t(o['rv0'].copy())
    y, sm, si = torch.native_batch_norm(x, w, b, rm, rv, True, MOMENTUM, EPS)
    if o['res'] is not None:
        y = y + t(o['res'])
    if o['relu']:
        y = torch.relu(y)
    y.backward(t(o['gy']))
    n = lambda a: None if a is None else a.detach().numpy()      # noqa: E731
    return dict(y=n(y), mean=n(sm), rstd=n(si), running_mean=n(rm), running_var=n(rv), gx=n(x.grad), gw=None if w is None else n(w.grad),
                gb=None if b is None else n(b.grad))


# ===================================================================================================================== LayerNorm
LnCase = collections.namedtuple('LnCase', 'name R C eps')


def ln_cases():
    return [LnCase('ln-R%d-C%d' % (R, Cn), R, Cn, (1e-6, 1e-5)[(i + j) % 2]) for i, R in enumerate(LN_R) for j, Cn in enumerate(LN_C)]


def ln_make(case):
    """row r: mu + sigma N(0, 1) with (mu, sigma) = PAIRS[r % 8]; rows r % 9 == 4: N(0, 1) with one 10^4 outlier"""
    rng = _rng(case.name)
    R, Cn = case.R, case.C
    mu, sg = np.array([PAIRS[r % 8][0] for r in range(R)])[:, None], np.array([PAIRS[r % 8][1] for r in range(R)])[:, None]
    x = mu + sg * rng.normal(0, 1, (R, Cn))
    for r in range(4, R, 9):
        x[r] = rng.normal(0, 1, Cn)
        x[r, Cn // 2] = 1e4
    e = (5 * np.arange(R)) % 17 - 8
    return dict(x=x.astype(F), w=rng.normal(0, 1, Cn).astype(F), b=rng.normal(0, 0.5, Cn).astype(F),
                gy=(rng.normal(0, 1, (R, Cn)) * 2.0 ** e[:, None]).astype(F), base_x=rng.normal(0, 1, (R, Cn)).astype(F),
                base_w=rng.normal(0, 1, Cn).astype(F), base_b=rng.normal(0, 1, Cn).astype(F))


def ln_fwd_ref(o, case):
    x = o['x'].astype(np.float64)
    mean, var, mbar = x.mean(1), x.var(1), np.abs(x).mean(1)
    S_var = var + U * C_MEAN ** 2 * mbar ** 2
    rstd = 1 / np.sqrt(var + case.eps)
    S_rstd = rstd * (1 + S_var / (2 * (var + case.eps)))
    w, b = o['w'].astype(np.float64), o['b'].astype(np.float64)
    xh = (x - mean[:, None]) * rstd[:, None]
    y = xh * w + b
    S = np.abs(w) * (rstd * mbar)[:, None] + 2 * np.abs(w * xh) + np.abs(y) + np.abs(b)
    return dict(y=(y, S), mean=(mean, mbar), rstd=(rstd, S_rstd))


def ln_bwd_ref(o, mean, rstd, accumulate_x=False, accumulate_wb=False):
    """analytic backward with the saved statistics as operands"""
    x, gy, w = (o[k].astype(np.float64) for k in ('x', 'gy', 'w'))
    Cn = x.shape[1]
    mean, rstd = np.asarray(mean, np.float64)[:, None], np.asarray(rstd, np.float64)[:, None]
    xh, gh = (x - mean) * rstd, gy * w
    s1, s2 = gh.mean(1, keepdims=True), (gh * xh).mean(1, keepdims=True)
    A1, A2 = np.abs(gh).mean(1, keepdims=True), 2 * np.abs(gh * xh).mean(1, keepdims=True)
    gx = rstd * (gh - s1 - xh * s2)
    Sx = rstd * (2 * np.abs(gh) + np.abs(s1) + A1 + np.abs(xh) * (2 * np.abs(s2) + A2)) + np.abs(gx)
    gw, Sw, gb, Sb = (gy * xh).sum(0), 2 * np.abs(gy * xh).sum(0), gy.sum(0), np.abs(gy).sum(0)
    if accumulate_x:
        gx, Sx = gx + o['base_x'], Sx + np.abs(o['base_x']) + np.abs(gx + o['base_x'])
    if accumulate_wb:
        gw, Sw = gw + o['base_w'], Sw + np.abs(o['base_w']) + np.abs(gw + o['base_w'])
        gb, Sb = gb + o['base_b'], Sb + np.abs(o['base_b']) + np.abs(gb + o['base_b'])
    return dict(gx=(gx, Sx), gw=(gw, Sw), gb=(gb, Sb))


def ln_fwd32(o, case, pad_mean=False):
    """float32 in the kernel's order (two passes in registers); pad_mean: the mean divided by 64 ceil(C / 64)"""
    x, Cn = o['x'], case.C
    div = F(64 * ((Cn + 63) // 64) if pad_mean else Cn)
    mean = (np.add.reduce(x, 1, dtype=F) / div).astype(F)
    d = x - mean[:, None]
    rs = (F(1) / np.sqrt(np.add.reduce(d * d, 1, dtype=F) / F(Cn) + F(case.eps))).astype(F)
    return dict(y=(d * rs[:, None] * o['w'] + o['b']).astype(F), mean=mean, rstd=rs)


def ln_bwd32(o, mean, rs):
    x, gy, w = o['x'], o['gy'], o['w']
    Cn = F(x.shape[1])
    xh, gh = (x - mean[:, None]) * rs[:, None], gy * w
    s1, s2 = np.add.reduce(gh, 1, dtype=F)[:, None] / Cn, np.add.reduce(gh * xh, 1, dtype=F)[:, None] / Cn
    return dict(gx=(rs[:, None] * (gh - s1 - xh * s2)).astype(F), gw=np.add.reduce(gy * xh, 0, dtype=F), gb=np.add.reduce(gy, 0, dtype=F))


def ln_torch32(o, case):
    x, w, b = (torch.from_numpy(o[k].copy()).requires_grad_(True) for k in ('x', 'w', 'b'))
    y, mean, rstd = torch.native_layer_norm(x, (case.C,), w, b, case.eps)
    y.backward(torch.from_numpy(o['gy']))
    return dict(y=y.detach().numpy(), mean=mean.detach().numpy().reshape(-1), rstd=rstd.detach().numpy().reshape(-1), gx=x.grad.numpy(),
                gw=w.grad.numpy(), gb=b.grad.numpy())


# ===================================================================================================================== attention
AttCase = collections.namedtuple('AttCase', 'name kind B T H')


def att_cases():
    return [AttCase('att-%s-B%d-T%d-H%d' % (k, B, T, H), k, B, T, H) for k in ATT_KINDS for T in ATT_T for H in ATT_H for B in ATT_B]


def att_make(case):
    """qkv [B, T, 3, H, 32] and gout [B, T, H 32]: 'normal' N(0, 1); 'large' q, k ~ 10 N(0, 1) (|logit| up to ~300: exp overflows without the max
    subtraction); 'onehot' q_i = 16 k_j(i) (one dominating key); 'uniform' all keys equal; 'qzero' q = 0"""
    rng = _rng(case.name)
    B, T, H, D = case.B, case.T, case.H, ATT_D
    qkv = rng.normal(0, 1, (B, T, 3, H, D))
    if case.kind == 'large':
        qkv[:, :, :2] *= 10.0
    elif case.kind == 'onehot':
        j = rng.randint(0, T, (B, T, H))
        for bi in range(B):
            for h in range(H):
                qkv[bi, :, 0, h] = 16.0 * qkv[bi, j[bi, :, h], 1, h]
    elif case.kind == 'uniform':
        qkv[:, :, 1] = qkv[:, :1, 1]
    elif case.kind == 'qzero':
        qkv[:, :, 0] = 0.0
    return dict(qkv=qkv.astype(F), gout=rng.normal(0, 1, (B, T, H * D)).astype(F), scale=D ** -0.5)


def _qkv64(o):
    return (o['qkv'].astype(np.float64).transpose(2, 0, 3, 1, 4)[j] for j in range(3))               # [B, H, T, D]


def att_fwd_ref(o, case):
    q, k, v = _qkv64(o)
    B, T, H, D = case.B, case.T, case.H, ATT_D
    sc = o['scale']
    s, SL = q @ k.transpose(0, 1, 3, 2) * sc, np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2) * sc
    mx = s.max(-1, keepdims=True)
    p = np.exp(s - mx)
    p /= p.sum(-1, keepdims=True)
    Sp = p * (SL + (p * SL).sum(-1, keepdims=True) + np.abs(s) + np.abs(s - mx) + 4)
    out, So = p @ v, (Sp + p) @ np.abs(v)
    tr = lambda a: a.transpose(0, 2, 1, 3).reshape(B * T, H * D)      # noqa: E731
    return dict(probs=(p, Sp), out=(tr(out), tr(So)))


def att_bwd_ref(o, case, probs):
    """-> gqkv [B T, 3 H 32] and its S, the saved probs as operands"""
    q, k, v = _qkv64(o)
    B, T, H, D = case.B, case.T, case.H, ATT_D
    sc, P = o['scale'], np.asarray(probs, np.float64)
    g = o['gout'].astype(np.float64).reshape(B, T, H, D).transpose(0, 2, 1, 3)
    Pt = P.transpose(0, 1, 3, 2)
    gv, Sv = Pt @ g, np.abs(Pt) @ np.abs(g)
    gP, SgP = g @ v.transpose(0, 1, 3, 2), np.abs(g) @ np.abs(v).transpose(0, 1, 3, 2)
    dot, Sdot = (gP * P).sum(-1, keepdims=True), ((SgP + np.abs(gP)) * np.abs(P)).sum(-1, keepdims=True)
    gS = P * (gP - dot) * sc
    SgS = sc * np.abs(P) * (SgP + Sdot + 2 * np.abs(gP - dot)) + 2 * np.abs(gS)
    gq, Sq = gS @ k, SgS @ np.abs(k)
    gk, Sk = gS.transpose(0, 1, 3, 2) @ q, SgS.transpose(0, 1, 3, 2) @ np.abs(q)
    pk = lambda a, b_, c_: np.stack([a, b_, c_]).transpose(1, 3, 0, 2, 4).reshape(B * T, 3 * H * D)      # noqa: E731
    return pk(gq, gk, gv), pk(Sq, Sk, Sv)


def att_fwd32(o, case, no_max=False, drop_last=False):
    q, k, v = (a.astype(F) for a in _qkv64(o))
    B, T, H, D = case.B, case.T, case.H, ATT_D
    s = (q @ k.transpose(0, 1, 3, 2) * F(o['scale'])).astype(F)
    if drop_last and T > 1:
        s, v = s[..., :-1], v[:, :, :-1]
    with np.errstate(over='ignore', invalid='ignore'):
        p = np.exp(s if no_max else s - s.max(-1, keepdims=True)).astype(F)
        p = (p / np.add.reduce(p, -1, dtype=F, keepdims=True)).astype(F)
        out = (p @ v).astype(F)
    if drop_last and T > 1:
        p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), F)], -1)
    return dict(probs=p, out=out.transpose(0, 2, 1, 3).reshape(B * T, H * D))


def att_bwd32(o, case, probs, gk_no_scale=False):
    q, k, v = (a.astype(F) for a in _qkv64(o))
    B, T, H, D = case.B, case.T, case.H, ATT_D
    sc, P = F(o['scale']), np.asarray(probs, F)
    g = o['gout'].reshape(B, T, H, D).transpose(0, 2, 1, 3)
    gv = P.transpose(0, 1, 3, 2) @ g
    gP = g @ v.transpose(0, 1, 3, 2)
    gS0 = (P * (gP - np.add.reduce(gP * P, -1, dtype=F, keepdims=True))).astype(F)
    gS = gS0 * sc
    gq, gk = gS @ k, (gS0 if gk_no_scale else gS).transpose(0, 1, 3, 2) @ q
    return np.stack([gq, gk, gv]).transpose(1, 3, 0, 2, 4).reshape(B * T, 3 * H * D).astype(F)


def att_torch32(o, case):
    B, T, H, D = case.B, case.T, case.H, ATT_D
    qkv = torch.from_numpy(o['qkv'].copy()).requires_grad_(True)
    q, k, v = (qkv.permute(2, 0, 3, 1, 4)[j] for j in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * o['scale'], -1)
    p.retain_grad()
    out = (p @ v).transpose(1, 2).reshape(B * T, H * D)
    out.backward(torch.from_numpy(o['gout']).reshape(B * T, H * D))
    return dict(probs=p.detach().numpy(), out=out.detach().numpy(), gqkv=qkv.grad.numpy().reshape(B * T, 3 * H * D))


# ===================================================================================================================== GELU
GeluCase = collections.namedtuple('GeluCase', 'name n')


def gelu_cases():
    return [GeluCase('gelu-n%d' % n, n) for n in (1, 255, 256, 257)] + [GeluCase('gelu-values', 2 * len(GELU_VALUES)), GeluCase('gelu-grid', 1 << 16)]


def gelu_make(case):
    """'values': +-GELU_VALUES; 'grid': 2^16 points spread evenly over [-7, 7]; n = ...: the first n of a fixed shuffle of both (2.0 first)"""
    vals = np.concatenate([np.array(GELU_VALUES), -np.array(GELU_VALUES)])
    grid = np.linspace(-7, 7, 1 << 16)
    rng = _rng(case.name)
    if case.name == 'gelu-values':
        x = vals
    elif case.name == 'gelu-grid':
        x = grid
    else:
        pool = np.concatenate([vals, grid[::257]])
        x = np.concatenate([[2.0], pool[_rng('gelu-shuffle').permutation(len(pool))]])[:case.n]
    e = (5 * np.arange(len(x))) % 17 - 8
    return dict(x=x.astype(F), gy=(rng.normal(0, 1, len(x)) * 2.0 ** e).astype(F))


def gelu_ref(o):
    x, gy = o['x'].astype(np.float64), o['gy'].astype(np.float64)
    er = erf(x / np.sqrt(2))
    with np.errstate(over='ignore', under='ignore'):
        pdf = np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)
        xp = np.where(pdf > 0, np.abs(x) * pdf, 0.0)
        y, Sy = 0.5 * x * (1 + er), 0.5 * np.abs(x) * (1 + np.abs(er))
        gx = gy * (0.5 * (1 + er) + np.where(pdf > 0, x * pdf, 0.0))
        Sg = np.abs(gy) * (0.5 * (1 + np.abs(er)) + np.where(pdf > 0, xp * (2 + np.minimum(x * x, 1e6)), 0.0)) + np.abs(gx)
    return dict(y=(y, Sy), gx=(gx, Sg))


def gelu32(o, tanh=False):
    x, gy = o['x'], o['gy']
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        if tanh:
            t = np.tanh(F(0.7978845608) * (x + F(0.044715) * x * x * x)).astype(F)
            cdf = F(0.5) * (F(1) + t)
            return dict(y=(x * cdf).astype(F), gx=(gy * (cdf + x * F(0.5) * (F(1) - t * t) * F(0.7978845608) * (F(1) + F(3 * 0.044715) * x * x))).astype(F))
        cdf = F(0.5) * (F(1) + erf(x * F(0.70710678118654752)).astype(F))
        pdf = F(0.39894228040143268) * np.exp(F(-0.5) * x * x).astype(F)
        return dict(y=(x * cdf).astype(F), gx=(gy * (cdf + x * pdf)).astype(F))


def gelu_torch32(o):
    x = torch.from_numpy(o['x'].copy()).requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.backward(torch.from_numpy(o['gy']))
    return dict(y=y.detach().numpy(), gx=x.grad.numpy())


# ===================================================================================================================== column sums
ColCase = collections.namedtuple('ColCase', 'name R N ld')


def colsum_cases():
    L = [ColCase('colsum-R%d-N%d' % (R, N), R, N, N) for R in COLSUM_R for N in COLSUM_N]
    L += [ColCase('colsum-R%d-N%d-ld%d' % (R, N, N + d), R, N, N + d) for R in (129, 513, 4097) for N in (4, 60) for d in (4, 1)]
    return L


def colsum_expected_kernels(case, accumulate):
    """dir_colsum_f32's dispatch restated (the buffers of the sweep are 16-byte aligned)"""
    R, N, ld = case.R, case.N, case.ld
    if 128 <= R <= 4096 and N >= 4 and N % 4 == 0 and ld % 4 == 0:
        return ['colsum_mid_kernel']
    if R <= BN_SMALL_R:
        return ['colsum_kernel']
    return ['bn_partial4_kernel' if N % 4 == 0 and ld % 4 == 0 else 'bn_partial_kernel', 'wgrad_reduce_kernel' if accumulate else 'bn_colsum_chunks_kernel']


def colsum_make(case):
    rng = _rng(case.name)
    mu, sg = np.array([PAIRS[c % 8][0] for c in range(case.N)]), np.array([PAIRS[c % 8][1] for c in range(case.N)])
    return dict(x=(mu + sg * rng.normal(0, 1, (case.R, case.N))).astype(F), base=rng.normal(0, 1, case.N).astype(F))


def colsum_ref(o, accumulate):
    x = o['x'].astype(np.float64)
    s, S = x.sum(0), np.abs(x).sum(0)
    if accumulate:
        s, S = s + o['base'], S + np.abs(o['base']) + np.abs(s + o['base'])
    return s, S


def colsum32(o, accumulate):
    x = o['x']
    if x.shape[0] <= BN_SMALL_R:
        s = np.add.reduce(x, 0, dtype=F)
    else:
        s = np.add.reduce(np.stack([np.add.reduce(x[a:a + BN_CHUNK], 0, dtype=F) for a in range(0, x.shape[0], BN_CHUNK)]), 0, dtype=F)
    return s + o['base'] if accumulate else s


# ===================================================================================================================== judges and stand-ins
FILL = 3.0            # what unwritten output elements hold (the sweep's canary value)


class Tally(object):
    """worst ratio per output kind and the failures of one run of a judge"""
    def __init__(self):
        self.ratios, self.failures, self.band = {}, [], 0.0

    def chk(self, kind, what, got, ref, S, chain):
        r = ratio(got, ref, np.broadcast_to(S, np.shape(ref)))
        if r >= self.ratios.get(kind, (-1.0, ''))[0]:
            self.ratios[kind] = (r, what)
        if not r <= c_eff(kind, chain):
            try:
                check(got, ref, np.broadcast_to(S, np.shape(ref)), c_eff(kind, chain), what)
            except AssertionError as e:
                self.failures.append(str(e))

    def merge(self, other):
        for k, v in other.ratios.items():
            if v[0] >= self.ratios.get(k, (-1.0, ''))[0]:
                self.ratios[k] = v
        self.failures += other.failures
        self.band = max(self.band, other.band)


def _rank_slices(case):
    r0 = np.cumsum((0,) + case.splits)
    return [slice(int(a), int(e)) for a, e in zip(r0[:-1], r0[1:])]


def bn_judge(case, variant, o, got):
    """every output of one BatchNorm case against its float64 reference.  got: y, mean, rstd [, var (sync), running_mean, running_var, pre_scale,
    pre_shift, gx, gw, gb] -- the backward ran on got's mean / rstd (for sync: gw / gb are [W, C], one row per rank).  -> Tally"""
    t, R, nm = Tally(), case.R, case.name + '/' + variant
    x64 = o['x'].astype(np.float64)
    w, b = o['w'], o['b']
    f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
    if case.api == 'frozen':
        mean, rstd = f64(o['rm0']), 1 / np.sqrt(f64(o['rv0']) + EPS)
        t.chk('bn_mean', nm + ' save_mean', got['mean'], mean, 0 * mean, R)
        t.chk('bn_rstd', nm + ' save_rstd', got['rstd'], rstd, 2 * rstd, R)
        pre, S = bn_y_ref(x64, w, b, mean, rstd, 0.0, o['res'])
    else:
        st = bn_stats_ref(x64, bn_levels(case), (o['p1'], o['p2']) if case.api == 'partials' else None)
        t.chk('bn_mean', nm + ' mean', got['mean'], st['mean'], st['S_mean'], R)
        if case.api == 'sync':
            t.chk('bn_var', nm + ' var', got['var'], st['var'], st['S_var'], R)
            mean, rstd = f64(got['mean']), 1 / np.sqrt(f64(got['var']) + EPS)
            t.chk('bn_rstd', nm + ' save_rstd', got['rstd'], rstd, 2 * rstd, R)
            pre, S = bn_y_ref(x64, w, b, mean, rstd, 0.0, o['res'])
        else:
            t.chk('bn_rstd', nm + ' rstd', got['rstd'], st['rstd'], st['S_rstd'], R)
            pre, S = bn_y_ref(x64, w, b, st['mean'], st['rstd'], st['S_mean'], o['res'])
        if got.get('running_mean') is not None:
            (rm, Srm), (rv, Srv) = bn_running_ref(st, o['rm0'], o['rv0'])
            t.chk('bn_running', nm + ' running_mean', got['running_mean'], rm, Srm, R)
            t.chk('bn_running', nm + ' running_var', got['running_var'], rv, Srv, R)
        if got.get('pre_scale') is not None:
            (k, Sk), (sh, Ssh) = bn_pre_ref(st, w, b)
            t.chk('bn_pre', nm + ' pre_scale', got['pre_scale'], k, Sk, R)
            t.chk('bn_pre', nm + ' pre_shift', got['pre_shift'], sh, Ssh, R)
    mask = None
    if o['relu']:
        yref, mask, band, wrong = relu_resolve(pre, S, c_eff('bn_y', R), got['y'])
        t.band = float(band.mean())
        if wrong.any():
            t.failures.append('%s: the ReLU mask differs from the float64 mask at %d elements off the undecided band' % (nm, int(wrong.sum())))
        if t.band > BAND_CAP:
            t.failures.append('%s: the undecided band holds %.3f %% of the elements' % (nm, 100 * t.band))
    else:
        yref = pre
    t.chk('bn_y', nm + ' y', got['y'], yref, S, R)
    if got.get('gw') is None:
        return t
    mk, rk = f64(got['mean']), f64(got['rstd'])
    full = bn_bwd_ref(o['gy'], x64, w, mk, rk, mask, frozen=case.api == 'frozen')
    if case.api == 'sync':
        for r, sl in enumerate(_rank_slices(case)):
            part = bn_bwd_ref(o['gy'][sl], x64[sl], w, mk, rk, None if mask is None else mask[sl], frozen=True)
            t.chk('bn_gb', nm + ' gb rank %d' % r, got['gb'][r], part['gb'][0], part['gb'][1], sl.stop - sl.start)
            t.chk('bn_gw', nm + ' gw rank %d' % r, got['gw'][r], part['gw'][0], part['gw'][1], sl.stop - sl.start)
    else:
        t.chk('bn_gb', nm + ' gb', got['gb'], full['gb'][0], full['gb'][1], R)
        t.chk('bn_gw', nm + ' gw', got['gw'], full['gw'][0], full['gw'][1], R)
    if got.get('gx') is not None:
        t.chk('bn_gx', nm + ' gx', got['gx'], full['gx'][0], full['gx'][1], R)
    return t


BN_DEFECTS = ('one_pass', 'drop_nkd2', 'last_full', 'biased_running', 'row_tail', 'quad_tail', 'mask_no_bias', 'padded_rows', 'sync_no_rank_mean')


def bn_defect_applies(defect, case, variant):
    """the cases a defect changes by more than a rounding"""
    chunked = case.api in ('train', 'split') and case.R > BN_SMALL_R
    bwd = variant != 'relu_res'
    return {'one_pass': case.api != 'frozen' and case.api != 'partials' and case.R >= 2 and case.C >= 2 and variant in ('plain', 'no_gx', 'no_wb'),
            'drop_nkd2': chunked or case.api == 'partials' or (case.api == 'sync' and case.R > 600),
            'last_full': (chunked and case.R % BN_CHUNK != 0) or (case.api == 'partials' and case.R % case.chunk_rows != 0),
            'biased_running': case.api not in ('frozen',) and case.R >= 2,
            'row_tail': case.R % 4 != 0 and case.R > 4,
            'quad_tail': case.C >= 4 and case.C % 16 != 0,
            'mask_no_bias': variant in ('relu', 'relu_res') and case.R >= 15,
            'padded_rows': chunked and case.R % BN_CHUNK != 0 and bwd and variant != 'no_gx',
            'sync_no_rank_mean': case.api == 'sync' and len(case.splits) > 1}[defect]


def bn_standin32(case, variant, o, defect=None):
    """the float32 numpy evaluation in the kernels' documented order, standing in for the kernels; defect: one of BN_DEFECTS"""
    lv, R, Cn = bn_levels(case), case.R, case.C
    if case.api == 'frozen':
        mean, var = o['rm0'], o['rv0']
    else:
        drop = {'drop_nkd2': tuple(range(len(lv))), 'sync_no_rank_mean': (len(lv) - 1,)}.get(defect, ())
        mean, var, _ = bn_stats32(o['x'], lv, (o['p1'], o['p2']) if case.api == 'partials' else None, one_pass=defect == 'one_pass', drop=drop,
                                  last_full=defect == 'last_full')
    got = bn_fwd32(o, case, mean, var, biased_running=defect == 'biased_running', mask_no_bias=defect == 'mask_no_bias')
    if case.api == 'sync':
        got['var'] = var
        unb = var * F(R) / F(R - 1) if defect != 'biased_running' else var
        got['running_var'] = (F(1) - F(MOMENTUM)) * o['rv0'] + F(MOMENTUM) * unb
    if case.api == 'frozen':
        got['running_mean'] = got['running_var'] = None
    if case.api not in ('split', 'partials'):
        got['pre_scale'] = got['pre_shift'] = None
    if defect == 'row_tail':
        got['y'][(R // 4) * 4:] = FILL
    if defect == 'quad_tail':
        got['y'][:, Cn - 4:] = FILL
    if variant == 'relu_res':
        return got
    mask = got['y'] > 0 if o['relu'] else None
    n_div = BN_CHUNK * ((R + BN_CHUNK - 1) // BN_CHUNK) if defect == 'padded_rows' else None
    bw = bn_bwd32(o, case, got['mean'], got['rstd'], mask, n_div, frozen=case.api == 'frozen')
    if case.api == 'sync':
        per = [bn_bwd32(dict(o, x=o['x'][sl], gy=o['gy'][sl]), case, got['mean'], got['rstd'], None if mask is None else mask[sl], frozen=True)
               for sl in _rank_slices(case)]
        bw['gb'], bw['gw'] = np.stack([p['gb'] for p in per]), np.stack([p['gw'] for p in per])
    if not o['need_gx']:
        bw['gx'] = None
    got.update(bw)
    return got


def bn_standin_torch(case, variant, o):
    """torch's own float32 operator as the stand-in (api 'train' and 'split', R > 1)"""
    got = bn_torch32(o, case)
    if variant == 'relu_res':
        got['gx'] = got['gw'] = got['gb'] = None
    if not o['need_gx']:
        got['gx'] = None
    if got['gw'] is None and variant != 'relu_res':                   # w / b absent: torch has no gradient for them; take the float32 sums
        mask = got['y'] > 0 if o['relu'] else None
        bw = bn_bwd32(o, case, got['mean'], got['rstd'], mask)
        got['gw'], got['gb'] = bw['gw'], bw['gb']
    return got


LN_MODES = ('plain', 'accumulate_x', 'accumulate_wb', 'no_gx')


def ln_judge(case, o, got, mode):
    """got: y, mean, rstd, gx (None under no_gx), gw, gb -- the backward ran on got's mean / rstd"""
    t, nm = Tally(), case.name + '/' + mode
    f = ln_fwd_ref(o, case)
    t.chk('ln_y', nm + ' y', got['y'], f['y'][0], f['y'][1], case.C)
    t.chk('ln_mean', nm + ' mean', got['mean'], f['mean'][0], f['mean'][1], case.C)
    t.chk('ln_rstd', nm + ' rstd', got['rstd'], f['rstd'][0], f['rstd'][1], case.C)
    bw = ln_bwd_ref(o, got['mean'], got['rstd'], mode == 'accumulate_x', mode == 'accumulate_wb')
    if got.get('gx') is not None:
        t.chk('ln_gx', nm + ' gx', got['gx'], bw['gx'][0], bw['gx'][1], case.C)
    t.chk('ln_gw', nm + ' gw', got['gw'], bw['gw'][0], bw['gw'][1], case.R)
    t.chk('ln_gb', nm + ' gb', got['gb'], bw['gb'][0], bw['gb'][1], case.R)
    return t


def ln_standin(case, o, mode, torch32=False, pad_mean=False):
    if torch32:
        got = ln_torch32(o, case)
    else:
        got = ln_fwd32(o, case, pad_mean)
        got.update(ln_bwd32(o, got['mean'], got['rstd']))
    if mode == 'accumulate_x':
        got['gx'] = got['gx'] + o['base_x']
    if mode == 'accumulate_wb':
        got['gw'], got['gb'] = got['gw'] + o['base_w'], got['gb'] + o['base_b']
    if mode == 'no_gx':
        got['gx'] = None
    return got


def att_judge(case, o, got):
    """got: probs [B, H, T, T], out [B T, H 32], gqkv [B T, 3 H 32] -- the backward ran on got's probs"""
    t, nm, n = Tally(), case.name, case.T + ATT_D
    f = att_fwd_ref(o, case)
    t.chk('att_probs', nm + ' probs', got['probs'], f['probs'][0], f['probs'][1], n)
    t.chk('att_out', nm + ' out', got['out'], f['out'][0], f['out'][1], n)
    g, Sg = att_bwd_ref(o, case, got['probs'])
    B, T, H, D = case.B, case.T, case.H, ATT_D
    g3, S3, q3 = (a.reshape(B * T, 3, H * D) for a in (g, Sg, np.asarray(got['gqkv'], np.float64)))
    for j, kind in enumerate(('att_gq', 'att_gk', 'att_gv')):
        t.chk(kind, nm + ' ' + kind, q3[:, j], g3[:, j], S3[:, j], n)
    return t


def att_standin(case, o, torch32=False, defect=None):
    if torch32:
        return att_torch32(o, case)
    got = att_fwd32(o, case, no_max=defect == 'no_max', drop_last=defect == 'drop_last')
    got['gqkv'] = att_bwd32(o, case, got['probs'], gk_no_scale=defect == 'gk_no_scale')
    return got


def att_defect_applies(defect, case):
    return {'no_max': case.kind == 'large' and case.T >= 21, 'drop_last': case.kind in ('normal', 'uniform', 'qzero') and case.T >= 2,
            'gk_no_scale': case.kind == 'normal' and case.T >= 2}[defect]


def gelu_judge(case, o, got):
    t, r = Tally(), gelu_ref(o)
    t.chk('gelu_y', case.name + ' y', got['y'], r['y'][0], r['y'][1], NO_CHAIN)
    t.chk('gelu_gx', case.name + ' gx', got['gx'], r['gx'][0], r['gx'][1], NO_CHAIN)
    return t


def colsum_judge(case, o, got, accumulate):
    t = Tally()
    s, S = colsum_ref(o, accumulate)
    t.chk('colsum', '%s%s' % (case.name, '/accumulate' if accumulate else ''), got, s, S, case.R)
    return t
