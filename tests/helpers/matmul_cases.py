"""Edge cases of the matrix-core half of the backward pass: dir_gemm_f32 / _grouped / _splitk and dir_conv2d_wgrad_f32 (csrc/train_ops.hip),
dir_conv2d_wgrad_f16x3 / _pre (csrc/wgrad_x3.hip).  Case lists, deterministic operands, float64 references, the per-element error scale S, the
check, the restated dispatch predicates and the float32 CPU references the constants come from.  CPU only (numpy):
tests/test_matmul_cases_ref.py proves the pieces here, tests/test_gpu_gemm_sweep.py and tests/test_gpu_wgrad_sweep.py point the kernels at them.

check(got, ref, S, kind, terms)     every element: |got - ref| <= c_eff 2^-24 S + 2^-149, c_eff = min(C[kind], terms + 2) (x3: min(C, 16)).
  S      = sum_k |a_k b_k| + |bias| + |C0| of the element (a weight gradient: the sum over the in-image pixels of that tap, + |gw0|).  An element
           whose every term lies in the padding has S = 0: it must be 0 to the last bit (2^-149 is the smallest positive float32).
  terms  = the number of products the element sums: terms + 2 roundings (bias, C0) is what a serial float32 sum guarantees.
  C      = 4 x RATIOS[kind], RATIOS the larger |ref32 - ref64| / (2^-24 S) of two float32 CPU references over the whole case list: (a) a serial
           k-ascending sum and (b) numpy's pairwise sum of the float32 products (np.add.reduce along the contiguous axis: a fixed order, no BLAS);
           split-K and the chunked gradients cut both at the documented chunk length and add the partials in chunk order.  4 is the project's
           margin for another, equally valid summation order (norm_cases.C, conv_cases.C).
  x3     RATIOS['x3'] = the distance of a CPU emulation of the split (numpy float16 hi = f16(v s), lo = f16(v s - hi), products hi hi + lo hi +
           hi lo, float32 accumulation, x 1 / (sx sg)) from float64, plus RATIOS['wgrad']; capped at conv_cases' guaranteed 2^-20 S (c = 16).
Nothing here is measured on a kernel.

Operands: mixed signs, magnitudes 2^-8 .. 2^9 inside every row (x3: 2^-4 .. 2^5, below); class 'rowscale' multiplies the rows of A by 1e-6 .. 1e4; positive operands
where whole taps lie in the padding.  Whatever a case does not own -- lda / ldb pad columns, the rows between batch entries and groups, the
channels outside a slice -- holds NaN: the kernels clamp their re-reads into the owned region, so none may reach an output.

The x3 operands span less, by the number format: the split keeps v s = hi + lo with lo a float16, whose spacing stops shrinking at 2^-24 (the
denormals).  A product then carries 2^-25 (|a| + |b|) + 3 2^-22 |a b| in scaled units, and that is within 2^-20 |a b| only while both scaled
operands are at least 2^-3 x 2/3.  pow2_in_scale puts the largest at [2^9, 2^10), the 'scales' class moves it down to [2^6, 2^7): 2^9 of range is
what the guarantee covers, so gy and x are drawn from 2^-4 .. 2^5 and the pre-activated x is built free of cancellation (wgrad_make)."""
import collections
import zlib

import numpy as np

F = np.float32
U = 2.0 ** -24
FLOOR = 2.0 ** -149
FILL = 3.0
X3_SPAN = 4.0                       # x3 operands span 2^-4 .. 2^5 (see the module docstring)
X3_CAP = 16.0                       # 2^-20 S in units of 2^-24 S (conv_cases.c_eff)
F16_MAX = 65504.0
GEMM_SPLIT_CHUNK = 64               # train_ops.hip
SMALL_GRID = 128                    # dir_gemm_f32: 64 x 64 grids of at most this many workgroups run on 32 x 32 tiles

# measured by tests/test_matmul_cases_ref.py (test_constants_are_derived_..., test_x3_constant_..., which pin them within 1 %), serial | pairwise:
# gemm 16.78 | 7.32 (K = 97 at 2^17 of range in a row), splitk 10.83 | 5.77, wgrad 9.775 | 6.06; x3 = 8.580 (the emulation) + 8.351 (the float32
# references cut at x3_nominal_chunks)
RATIOS = {'gemm': 16.78, 'splitk': 10.83, 'wgrad': 9.775, 'x3': 16.93}
C = {k: 4.0 * v for k, v in RATIOS.items()}

TA_TB = ((0, 0), (0, 1), (1, 0), (1, 1))
MN_VALUES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 80, 81, 127, 129)
K_VALUES = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 97)
SPLITK_K = (1, 63, 64, 65, 128, 129, 2050)
GEMM_CLASSES = ('tails', 'grid', 'strides', 'rowscale', 'grouped', 'splitk')
GEMM_COUNTS = {'tails': 25, 'grid': 8, 'strides': 14, 'rowscale': 4, 'grouped': 20, 'splitk': 12}
GEMM_EXPECTED = {'tails': ('gemm_f32_small_kernel',), 'grid': ('gemm_f32_small_kernel', 'gemm_f32_kernel'),
                 'strides': ('gemm_f32_small_kernel', 'gemm_f32_kernel'), 'rowscale': ('gemm_f32_small_kernel',),
                 'grouped': ('gemm_f32_grouped_kernel', 'gemm_f32_grouped_short_kernel'),
                 'splitk': ('gemm_f32_small_kernel', 'gemm_f32_kernel', 'gemm_splitk_reduce_kernel')}

G = collections.namedtuple('G', 'name cls api M N K ta tb batch pa pb pc mis sb0 gapa gapc bias acc ny nx reduce neg rowscale')


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _g(cls, label, api, M, N, K, t, batch=1, pa=0, pb=0, pc=0, mis=0, sb0=False, gapa=0, gapc=0, bias=False, acc=False, ny=1, nx=1, reduce=0,
       neg=0, rowscale=False):
    return G('%s-%s_t%d%d' % (cls, label, t[0], t[1]), cls, api, M, N, K, t[0], t[1], batch, pa, pb, pc, mis, sb0, gapa, gapc, bias, acc, ny, nx,
             reduce, neg, rowscale)


def gemm_cases(cls, t):
    """the cases of one class at one (trans_a, trans_b)"""
    out = []
    if cls == 'tails':
        L = len(MN_VALUES)
        for i, M in enumerate(MN_VALUES):                        # every M with another N; every K twice or more
            out.append(_g(cls, 'M%d_N%d_K%d' % (M, MN_VALUES[(5 * i + 3) % L], K_VALUES[i % 11]), 'gemm', M, MN_VALUES[(5 * i + 3) % L],
                          K_VALUES[i % 11], t, bias=i % 2 == 1, acc=i % 3 == 2))
        for i, K in enumerate(K_VALUES):
            M, N = MN_VALUES[(3 * i + 1) % L], MN_VALUES[(7 * i + 2) % L]
            out.append(_g(cls, 'K%d_M%d_N%d' % (K, M, N), 'gemm', M, N, K, t, bias=i % 2 == 0, acc=i % 3 == 1))
    elif cls == 'grid':                                          # tiles x batch = 128 | 129 (and 132): the last small grid, the first large one
        for M, N, batch in ((64, 64, 128), (64, 64, 129), (65, 65, 32), (65, 65, 33), (129, 1, 42), (129, 1, 43), (33, 129, 43), (1, 127, 64)):
            out.append(_g(cls, 'M%d_N%d_b%d' % (M, N, batch), 'gemm', M, N, 5 if batch > 100 else 33, t, batch=batch, sb0=batch % 2 == 1,
                          bias=batch % 3 == 0, acc=batch % 4 == 1))
    elif cls == 'strides':
        out += [_g(cls, 'ld_pads', 'gemm', 33, 17, 35, t, pa=3, pb=5, pc=7, bias=True),
                _g(cls, 'ld_pads_acc', 'gemm', 65, 31, 64, t, pa=1, pb=1, pc=1, acc=True),
                _g(cls, 'mis_a', 'gemm', 32, 32, 33, t, mis=1, bias=True, acc=True),
                _g(cls, 'mis_b', 'gemm', 17, 64, 32, t, mis=2),
                _g(cls, 'mis_c', 'gemm', 64, 15, 31, t, mis=4, acc=True),
                _g(cls, 'mis_all_pads', 'gemm', 63, 33, 65, t, pa=2, pb=3, pc=5, mis=7, bias=True, acc=True),
                _g(cls, 'shared_b', 'gemm', 31, 33, 17, t, batch=3, sb0=True, bias=True),
                _g(cls, 'batch_gaps', 'gemm', 17, 16, 4, t, batch=4, gapa=7, gapc=9, pc=2, acc=True),
                _g(cls, 'big_shared_b', 'gemm', 65, 65, 33, t, batch=33, sb0=True, pa=1, pc=3, gapc=5, bias=True, acc=True),
                _g(cls, 'big_gaps', 'gemm', 64, 129, 5, t, batch=44, gapa=3, gapc=2, pb=1, mis=5),
                _g(cls, 'big_mis', 'gemm', 129, 127, 31, t, batch=22, mis=7, pa=3, pb=3, pc=3, bias=True),
                _g(cls, 'big_plain', 'gemm', 63, 65, 97, t, batch=65, acc=True),
                _g(cls, 'bias_only', 'gemm', 80, 81, 3, t, bias=True),
                _g(cls, 'none', 'gemm', 81, 80, 63, t)]
    elif cls == 'rowscale':
        out += [_g(cls, 'M64_N33', 'gemm', 64, 33, 65, t, rowscale=True, bias=True),
                _g(cls, 'M129_N17', 'gemm', 129, 17, 31, t, rowscale=True),
                _g(cls, 'M17_N64_acc', 'gemm', 17, 64, 97, t, rowscale=True, acc=True, pa=2),
                _g(cls, 'M81_N5', 'gemm', 81, 5, 33, t, rowscale=True, batch=2)]
    elif cls == 'grouped':
        for M in (64, 65, 79, 80, 81):                           # the 80-row tile serves 65 .. 80, both reduce modes
            for reduce in (0, 1):
                out.append(_g(cls, 'M%d_r%d' % (M, reduce), 'grouped', M, 33 + 32 * reduce, 33, t, ny=1 + 2 * reduce, nx=3, reduce=reduce,
                              bias=M % 2 == 1, acc=M in (65, 80), pc=M % 3))
        out += [_g(cls, 'one_group', 'grouped', 33, 65, 31, t, bias=True),
                _g(cls, 'one_group_80', 'grouped', 80, 17, 5, t, batch=3, gapa=3, gapc=1),
                _g(cls, 'neg_a_reduce', 'grouped', 72, 33, 21, t, ny=3, nx=3, reduce=1, neg=1, bias=True, acc=True),
                _g(cls, 'neg_a_side', 'grouped', 129, 16, 37, t, ny=3, nx=3, reduce=0, neg=1, pc=2),
                _g(cls, 'neg_b_reduce', 'grouped', 80, 65, 35, t, ny=3, nx=3, reduce=1, neg=2, bias=True),
                _g(cls, 'neg_b_side', 'grouped', 17, 80, 63, t, ny=1, nx=3, reduce=0, neg=2, acc=True, batch=2),
                _g(cls, 'reduce_tail_k1', 'grouped', 31, 31, 1, t, ny=3, nx=3, reduce=1, bias=True, acc=True),
                _g(cls, 'reduce_tail_k65', 'grouped', 66, 15, 65, t, ny=1, nx=3, reduce=1, acc=True, mis=7, pa=1, pb=2),
                _g(cls, 'side_batch', 'grouped', 15, 64, 32, t, ny=3, nx=3, reduce=0, batch=2, gapc=6, bias=True),
                _g(cls, 'side_mis', 'grouped', 75, 63, 4, t, ny=1, nx=3, reduce=0, mis=7, pa=3, pb=1, pc=1, acc=True)]
    elif cls == 'splitk':
        for i, K in enumerate(SPLITK_K):
            out.append(_g(cls, 'K%d' % K, 'splitk', (33, 64, 17, 65)[i % 4], (65, 31, 64, 16)[i % 4], K, t, bias=i % 2 == 0, acc=i % 3 == 0,
                          pc=(0, 3)[i % 2], pa=i % 2, pb=i % 3))
        out += [_g(cls, 'K8256_small_grid', 'splitk', 33, 17, 64 * 129 - 64, t, bias=True),     # 128 chunks on one tile: the last small grid
                _g(cls, 'K8256', 'splitk', 64, 63, 64 * 129, t, acc=True, pc=1),                  # 129 chunks: the first large one
                _g(cls, 'big_grid', 'splitk', 129, 129, 960, t, bias=True, acc=True, pc=5),       # 9 tiles x 15 chunks
                _g(cls, 'big_grid_mis', 'splitk', 127, 65, 2049, t, mis=7, pa=1, pb=1, bias=True),  # 4 tiles x 33 chunks (a 1-term last chunk)
                _g(cls, 'small_grid_mis', 'splitk', 15, 129, 193, t, mis=7, acc=True)]
    else:
        raise KeyError(cls)
    return out


def all_gemm_cases():
    return [c for cls in GEMM_CLASSES for t in TA_TB for c in gemm_cases(cls, t)]


def gemm_expected(c):
    """the kernels the entry point launches for the case, in order (the launch rules of train_ops.hip restated)"""
    tiles = -(-c.N // 64) * -(-c.M // 64)
    if c.api == 'gemm':
        return ['gemm_f32_small_kernel' if tiles * c.batch <= SMALL_GRID else 'gemm_f32_kernel']
    if c.api == 'grouped':
        return ['gemm_f32_grouped_short_kernel' if 64 < c.M <= 80 else 'gemm_f32_grouped_kernel']
    chunks = -(-c.K // GEMM_SPLIT_CHUNK)
    return ['gemm_f32_small_kernel' if tiles * chunks <= SMALL_GRID else 'gemm_f32_kernel', 'gemm_splitk_reduce_kernel']


def _vals(rng, n, positive=False, span=8.0):
    v = (1.0 + rng.rand(n)) * 2.0 ** rng.uniform(-span, span, n)
    return (v if positive else v * rng.choice((-1.0, 1.0), n)).astype(F)


GemmLayout = collections.namedtuple('GemmLayout', 'lda ldb ldc sA sB sC a_y a_x b_y b_x c_y c_x a0 b0 idxA idxB idxC nA nB nC')


def gemm_layout(c):
    """leading dimensions, strides, displacements and the flat index of every owned element: idxA [batch, groups, M, K], idxB [batch, groups, K, N]
    (transposes undone), idxC [batch, groups (1 with reduce), M, N]; a0 / b0: the offset of the pointer handed to the library"""
    ng = c.ny * c.nx
    ra, ca = (c.K, c.M) if c.ta else (c.M, c.K)
    rb, cb = (c.N, c.K) if c.tb else (c.K, c.N)
    lda, ldb = ca + c.pa, cb + c.pb
    side = c.api == 'grouped' and not c.reduce
    ldc = (c.nx * c.N if side else c.N) + c.pc

    def shifts(ext, ld, negative):
        if ng == 1:
            return 0, 0, 0, 0
        if negative:                                              # a tap as a pointer shift: one row per x step, three per y step, backwards
            return -3 * ld, -ld, (3 * (c.ny - 1) + (c.nx - 1)) * ld, (3 * (c.ny - 1) + (c.nx - 1)) * ld
        return c.nx * (ext + 5), ext + 5, 0, (ng - 1) * (ext + 5)
    a_y, a_x, a0, span_a = shifts(ra * lda, lda, c.neg == 1)
    b_y, b_x, b0, span_b = shifts(rb * ldb, ldb, c.neg == 2)
    sA = ra * lda + span_a + c.gapa
    sB = 0 if c.sb0 else rb * ldb + span_b + c.gapa
    c_y, c_x = (c.M * ldc, c.N) if side else (0, 0)
    sC = (c.ny if side else 1) * c.M * ldc + c.gapc
    bz = np.arange(c.batch, dtype=np.int64)[:, None, None, None]
    gy, gx = np.divmod(np.arange(ng, dtype=np.int64), c.nx)
    r_, c_ = np.arange(max(ra, rb, c.M), dtype=np.int64)[:, None], np.arange(max(ca, cb, c.N), dtype=np.int64)[None, :]
    idxA = a0 + bz * sA + (gy * a_y + gx * a_x)[None, :, None, None] + (r_[:ra] * lda + c_[:, :ca])[None, None]
    idxB = b0 + bz * sB + (gy * b_y + gx * b_x)[None, :, None, None] + (r_[:rb] * ldb + c_[:, :cb])[None, None]
    gc = (gy * c_y + gx * c_x) if side else np.zeros(1, np.int64)
    idxC = bz * sC + gc[None, :, None, None] + (r_[:c.M] * ldc + c_[:, :c.N])[None, None]
    if c.ta:
        idxA = idxA.transpose(0, 1, 3, 2)
    if c.tb:
        idxB = idxB.transpose(0, 1, 3, 2)
    assert idxA.min() >= 0 and idxB.min() >= 0 and np.unique(idxC).size == idxC.size
    return GemmLayout(lda, ldb, ldc, sA, sB, sC, a_y, a_x, b_y, b_x, c_y, c_x, a0, b0, idxA, idxB, idxC, int(idxA.max()) + 1 + c.pa, int(idxB.max()) + 1 + c.pb,
                      int(idxC.max()) + 1 + c.pc)          # (the last row's pad columns belong to the buffer)


def gemm_make(c):
    """-> dict: the layout L, flat operand buffers a / b (NaN where nothing is owned), bias, c0 (FILL where nothing is owned; the prefilled C of an
    accumulate case), and the operand matrices A [batch, groups, M, K], B [batch, groups, K, N] as float32"""
    rng, L = _rng(c.name), gemm_layout(c)
    a, b = _vals(rng, L.nA), _vals(rng, L.nB)
    if c.neg == 1:
        a[(np.arange(L.nA) // L.lda) % 4 == 0] = 0.0              # the zero border of the pixel grid the taps walk over
    if c.neg == 2:
        b[(np.arange(L.nB) // L.ldb) % 4 == 0] = 0.0
    if c.rowscale:
        s = (10.0 ** np.linspace(-6.0, 4.0, c.M))[rng.permutation(c.M)]
        a[L.idxA] = (a[L.idxA].astype(np.float64) * s[None, None, :, None]).astype(F)
    for buf, idx in ((a, L.idxA), (b, L.idxB)):
        own = np.zeros(buf.size, bool)
        own[idx.ravel()] = True
        buf[~own] = np.nan
    bias = _vals(rng, c.N) if c.bias else None
    c0 = np.full(L.nC, FILL, F)
    if c.acc:
        c0[L.idxC.ravel()] = _vals(rng, L.idxC.size)
    return dict(L=L, a=a, b=b, bias=bias, c0=c0, A=a[L.idxA], B=b[L.idxB])


def gemm_reference(c, o, A=None, B=None, bias_times=1):
    """float64: (ref, S, terms) in the shape of idxC"""
    A, B = (o['A'] if A is None else A).astype(np.float64), (o['B'] if B is None else B).astype(np.float64)
    ref, S = np.matmul(A, B), np.matmul(np.abs(A), np.abs(B))
    terms = c.K
    if c.api == 'grouped' and c.reduce:
        ref, S, terms = ref.sum(1, keepdims=True), S.sum(1, keepdims=True), c.K * c.ny * c.nx
    if c.bias:
        ref, S = ref + bias_times * o['bias'].astype(np.float64), S + np.abs(o['bias'].astype(np.float64))
    if c.acc:
        c0 = o['c0'][o['L'].idxC].astype(np.float64)
        ref, S = ref + c0, S + np.abs(c0)
    return ref, S, terms


# ----------------------------------------------------------------------------------------------------- float32 CPU references
def sum_serial(P, Q, acc=None):
    """sum_k P[k, :, None] Q[k, None, :] in float32, k ascending, one rounding per product and per addition"""
    P, Q = np.ascontiguousarray(P, F), np.ascontiguousarray(Q, F)
    acc = np.zeros((P.shape[1], Q.shape[1]), F) if acc is None else acc
    for k in range(P.shape[0]):
        acc += P[k][:, None] * Q[k][None, :]
    return acc


def sum_pairwise(P, Q):
    """the same sum as numpy's pairwise reduction of the float32 products along the contiguous axis (np.add.reduce: a fixed order, no BLAS)"""
    Pt, Qt = np.ascontiguousarray(np.asarray(P, F).T), np.ascontiguousarray(np.asarray(Q, F).T)
    out = np.empty((Pt.shape[0], Qt.shape[0]), F)
    step = max(1, (1 << 22) // max(1, Qt.shape[0] * Qt.shape[1]))
    for p0 in range(0, Pt.shape[0], step):
        out[p0:p0 + step] = np.add.reduce(Pt[p0:p0 + step, None, :] * Qt[None, :, :], axis=-1, dtype=F)
    return out


def chunked(P, Q, chunk, summer):
    """partials of `chunk` reduction rows each (an empty trailing chunk gives zeros), added in chunk order starting from 0"""
    s = np.zeros((P.shape[1], Q.shape[1]), F)
    for k0 in range(0, max(P.shape[0], 1), chunk):
        s = s + summer(P[k0:k0 + chunk], Q[k0:k0 + chunk])
    return s


def gemm_float32(c, o, how):
    """the case in float32 on the CPU, how = 'serial' | 'pairwise', in the kernels' documented order: groups in order inside one accumulation,
    split-K partials of 64 added in chunk order, then + bias, then C0 + (...)"""
    L, out = o['L'], np.zeros(o['L'].idxC.shape, F)
    for b in range(c.batch):
        for g in range(out.shape[1]):
            gs = range(c.ny * c.nx) if (c.api == 'grouped' and c.reduce) else (g,)
            if c.api == 'splitk':
                r = chunked(o['A'][b, g].T, o['B'][b, g], GEMM_SPLIT_CHUNK, sum_serial if how == 'serial' else sum_pairwise)
            elif how == 'serial':
                r = None
                for gg in gs:
                    r = sum_serial(o['A'][b, gg].T, o['B'][b, gg], r)
            else:
                r = sum_pairwise(np.concatenate([o['A'][b, gg].T for gg in gs]), np.concatenate([o['B'][b, gg] for gg in gs]))
            if c.bias:
                r = r + o['bias'][None, :]
            out[b, g] = o['c0'][L.idxC[b, g]] + r if c.acc else r
    return out


# ----------------------------------------------------------------------------------------------------- the check
def c_eff(kind, terms):
    return np.minimum(C[kind], X3_CAP if kind == 'x3' else np.asarray(terms, np.float64) + 2.0)


def tol(S, kind, terms):
    return c_eff(kind, terms) * U * np.asarray(S, np.float64) + FLOOR


def ratio(got, ref, S):
    """max (|got - ref| - 2^-149) / (2^-24 S) over the elements (0 where that is <= 0; inf for a non-finite got or an error where S = 0)"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    if not np.isfinite(got).all():
        return float('inf')
    e = np.maximum(np.abs(got - ref) - FLOOR, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e > 0, e / (U * S), 0.0)
    return float(r.max()) if r.size else 0.0


def check(got, ref, S, kind, terms, what=''):
    """every element |got - ref| <= tol(element); -> the largest ratio in units of 2^-24 S"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= np.broadcast_to(tol(S, kind, terms), ref.shape))            # (a NaN compares false: bad)
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError('%s: %d of %d elements outside their bound (kind %s, worst ratio %.4g of c = %.4g); first at %s: got %.9g, ref %.9g, '
                             'S %.4g' % (what, int(bad.sum()), bad.size, kind, ratio(got, ref, S), C[kind], i, got[i], ref[i], S[i]))
    return ratio(got, ref, S)


# ======================================================================================================= weight gradients
W = collections.namedtuple('W', 'name cls api B H W Cin Cout kh kw stride pad Ho Wo in_cs in_coff out_cs out_coff misx misg acc positive pre '
                                'shift gymag')
WGRAD_CLASSES = ('dispatch', 'chunks', 'geometry', 'slices')
WGRAD_VARIANTS = ('write', 'accumulate')
WGRAD_COUNTS = {'dispatch': 17, 'chunks': 14, 'geometry': 15, 'slices': 8}
X3_CLASSES = ('row32', 'row4', 'row0', 'magic', 'scales')
X3_VARIANTS = ('plain', 'lin', 'relu')
X3_COUNTS = {'row32': 14, 'row4': 15, 'row0': 15, 'magic': 7, 'scales': 9}
WGRAD_EXPECTED = {'dispatch': ('conv_wgrad_kernel', 'conv_wgrad4_kernel', 'conv_wgrad_flatk_kernel'),
                  'chunks': ('conv_wgrad_kernel', 'conv_wgrad4_kernel', 'conv_wgrad_flatk_kernel', 'wgrad_reduce_kernel'),
                  'geometry': ('conv_wgrad_kernel', 'conv_wgrad4_kernel', 'conv_wgrad_flatk_kernel'),
                  'slices': ('conv_wgrad_kernel', 'conv_wgrad4_kernel')}
X3_TILES = ((64, 64), (64, 128), (128, 64), (128, 128))
X3_FORMS = {'row32': 32, 'row4': 4, 'row0': 0}


def _w(cls, label, api, B, H, Wd, Cin, Cout, k=1, stride=1, pad=0, out=None, inx=(0, 0), outx=(0, 0), misx=False, misg=False, acc=False,
       positive=False, pre='', shift=0, gymag=1.0):
    kh, kw = (k, k) if isinstance(k, int) else k
    Ho, Wo = out or ((H + 2 * pad - kh) // stride + 1, (Wd + 2 * pad - kw) // stride + 1)
    return W('%s-%s' % (cls, label), cls, api, B, H, Wd, Cin, Cout, kh, kw, stride, pad, Ho, Wo, Cin + inx[0], inx[1], Cout + outx[0], outx[1],
             misx, misg, acc, positive, pre, shift, gymag)


def wgrad_cases(cls, variant):
    """dir_conv2d_wgrad_f32: the cases of a class; variant 'accumulate' adds onto a prefilled gw"""
    a = dict(acc=variant == 'accumulate')
    f = lambda *p, **k: _w(cls, *p, **dict(a, **k))      # noqa: E731
    if cls == 'dispatch':
        return [f('scalar_cin18', 'f32', 1, 5, 7, 18, 8, 3, 1, 1), f('scalar_cout6', 'f32', 2, 4, 4, 8, 6, 1),
                f('scalar_coff2', 'f32', 1, 6, 5, 16, 8, 3, 1, 1, inx=(4, 2)), f('scalar_misx', 'f32', 1, 6, 6, 16, 8, 3, 1, 1, misx=True),
                f('scalar_misg', 'f32', 1, 6, 6, 16, 8, 1, misg=True), f('scalar_gycoff2', 'f32', 1, 4, 9, 16, 4, 1, outx=(4, 2)),
                f('scalar_65', 'f32', 1, 3, 5, 65, 67, 3, 1, 1), f('scalar_cin15_k1', 'f32', 2, 5, 5, 15, 8, 1),
                f('vector_8', 'f32', 1, 6, 6, 8, 8, 1), f('vector_64', 'f32', 1, 5, 7, 64, 64, 1), f('vector_68_132', 'f32', 1, 4, 5, 68, 132, 3, 1, 1),
                f('vector_cin16_k3', 'f32', 1, 7, 6, 16, 12, 3, 1, 1), f('vector_cin4_k1', 'f32', 3, 3, 3, 4, 4, 1),
                f('flat_stem', 'f32', 1, 17, 19, 3, 8, 7, 2, 3), f('flat_cin15', 'f32', 1, 6, 5, 15, 9, 3, 1, 1),
                f('flat_cin1', 'f32', 2, 5, 5, 1, 65, 3, 1, 1), f('flat_cin4_aligned', 'f32', 1, 6, 6, 4, 8, 3, 1, 1)]
    if cls == 'chunks':
        out = []
        for M, (B, H, Wd) in ((255, (1, 15, 17)), (256, (1, 16, 16)), (257, (257, 1, 1)), (513, (1, 27, 19))):
            out += [f('vector_M%d' % M, 'f32', B, H, Wd, 8, 8, 1), f('scalar_M%d' % M, 'f32', B, H, Wd, 6, 5, 1),
                    f('flat_M%d' % M, 'f32', B, H, Wd, 3, 8, 3, 1, 1)]
        return out + [f('empty_last_chunk', 'f32', 2, 35, 55, 16, 452, 3, 1, 1),            # 15 chunks of 288: the 15th starts at 4032 > M = 3850
                      f('odd_steps_k3', 'f32', 1, 20, 24, 64, 64, 3, 1, 1)]                  # M = 480, 2 chunks of 256 | 224 (7 steps)
    if cls == 'geometry':
        p = dict(positive=True)
        return [f('s2_p0', 'f32', 1, 9, 11, 16, 8, 3, 2, 0), f('s2_p1', 'f32', 2, 8, 10, 16, 8, 3, 2, 1), f('s2_k1', 'f32', 1, 9, 9, 6, 8, 1, 2, 0),
                f('p2_k3', 'f32', 1, 5, 6, 20, 12, 3, 1, 2), f('p2_k5_flat', 'f32', 1, 6, 6, 3, 8, 5, 1, 2),
                f('pad3_2x2_vector', 'f32', 2, 2, 2, 16, 8, 3, 1, 3, out=(2, 2), **p), f('pad3_2x2_scalar', 'f32', 2, 2, 2, 17, 5, 3, 1, 3, out=(2, 2), **p),
                f('pad3_2x2_flat', 'f32', 2, 2, 2, 3, 8, 3, 1, 3, out=(2, 2), **p),
                f('k1x3', 'f32', 1, 5, 8, 16, 8, (1, 3), 1, 1), f('k3x1', 'f32', 1, 8, 5, 18, 7, (3, 1), 1, 1), f('k1x3_flat', 'f32', 1, 4, 9, 5, 8, (1, 3), 1, 0),
                f('h1', 'f32', 3, 1, 13, 16, 8, 3, 1, 1, **p), f('w1', 'f32', 3, 13, 1, 7, 8, 3, 1, 1, **p),
                f('out_smaller', 'f32', 1, 9, 9, 32, 8, 3, 1, 1, out=(7, 5)), f('out_smaller_s2_flat', 'f32', 2, 11, 11, 3, 16, 3, 2, 1, out=(4, 5))]
    if cls == 'slices':
        return [f('vector_in', 'f32', 1, 6, 6, 16, 8, 3, 1, 1, inx=(8, 4)), f('vector_out', 'f32', 1, 6, 6, 8, 8, 1, outx=(12, 8)),
                f('vector_both', 'f32', 2, 5, 7, 64, 68, 3, 1, 1, inx=(4, 4), outx=(8, 4)), f('vector_both_chunked', 'f32', 1, 17, 17, 8, 8, 1, inx=(4, 0), outx=(4, 4)),
                f('scalar_in', 'f32', 1, 6, 6, 16, 8, 3, 1, 1, inx=(3, 1)), f('scalar_out', 'f32', 1, 6, 6, 8, 8, 1, outx=(5, 3)),
                f('scalar_both', 'f32', 2, 5, 7, 17, 6, 3, 1, 1, inx=(3, 2), outx=(2, 1)), f('scalar_both_chunked', 'f32', 1, 17, 17, 6, 8, 1, inx=(2, 2), outx=(4, 2))]
    raise KeyError(cls)


def x3_cases(cls, variant):
    """dir_conv2d_wgrad_f16x3 (variant 'plain') / _pre ('lin': x <- x s + b, 'relu': max(x s + b, 0))"""
    a = dict(pre='' if variant == 'plain' else variant)
    f = lambda *p, **k: _w(cls, *p, **dict(a, **k))      # noqa: E731
    if cls == 'row32':                                           # Wo % 32 == 0
        return [f('64x64_full', 'x3', 1, 2, 32, 64, 64, 3, 1, 1), f('64x64_36_32', 'x3', 1, 3, 32, 36, 32, 1), f('64x64_s2_k3', 'x3', 1, 4, 64, 32, 36, 3, 2, 1),
                f('64x128_full', 'x3', 1, 1, 32, 128, 64, 1), f('64x128_68', 'x3', 1, 2, 32, 68, 36, 3, 1, 1), f('64x128_s2_k1', 'x3', 2, 3, 64, 132, 32, 1, 2, 0),
                f('128x64_full', 'x3', 1, 2, 32, 64, 128, 1), f('128x64_68', 'x3', 1, 3, 32, 32, 68, 3, 1, 1, acc=True), f('128x64_260', 'x3', 1, 1, 32, 36, 260, 1),
                f('128x128_full', 'x3', 1, 1, 32, 128, 128, 1), f('128x128_68', 'x3', 1, 2, 32, 68, 68, 3, 1, 1), f('128x128_260_132', 'x3', 1, 1, 32, 260, 132, 1),
                f('chunked_32x32', 'x3', 2, 32, 32, 64, 64, 1), f('chunked_32x32_k3', 'x3', 2, 32, 32, 36, 64, 3, 1, 1, acc=True)]
    if cls == 'row4':                                            # Wo % 4 == 0, not 32
        return [f('64x64_wo4', 'x3', 1, 4, 4, 64, 64, 3, 1, 1), f('64x64_wo12', 'x3', 1, 5, 12, 36, 32, 3, 1, 1), f('64x64_one_step', 'x3', 2, 4, 4, 32, 36, 1),
                f('64x128_wo4', 'x3', 3, 2, 4, 128, 64, 1), f('64x128_wo12', 'x3', 1, 8, 12, 68, 36, 3, 1, 1), f('64x128_s2', 'x3', 1, 7, 24, 132, 32, 3, 2, 1),
                f('128x64_wo4', 'x3', 1, 1, 4, 64, 128, 1), f('128x64_wo12', 'x3', 1, 2, 12, 32, 68, 3, 1, 1, acc=True), f('128x64_260', 'x3', 1, 3, 4, 36, 260, 1),
                f('128x128_wo4', 'x3', 1, 5, 4, 128, 128, 1), f('128x128_three_steps', 'x3', 1, 8, 12, 68, 68, 3, 1, 1), f('128x128_260', 'x3', 1, 2, 4, 260, 260, 3, 1, 1),
                f('chunked_12x12', 'x3', 8, 12, 12, 64, 64, 3, 1, 1), f('chunked_12x12_acc', 'x3', 8, 12, 12, 36, 68, 1, acc=True),
                f('out_smaller', 'x3', 1, 9, 9, 32, 32, 3, 1, 1, out=(7, 4))]
    if cls == 'row0':                                            # neither
        return [f('64x64_wo1', 'x3', 3, 7, 1, 64, 64, 3, 1, 1), f('64x64_wo5', 'x3', 1, 5, 5, 36, 32, 3, 1, 1), f('64x64_wo13', 'x3', 1, 13, 13, 32, 36, 1),
                f('64x128_wo5', 'x3', 1, 6, 5, 128, 64, 1), f('64x128_wo13', 'x3', 1, 5, 13, 68, 36, 3, 1, 1), f('64x128_s2', 'x3', 1, 9, 10, 132, 32, 3, 2, 1),
                f('128x64_wo1', 'x3', 33, 1, 1, 64, 128, 1), f('128x64_wo5', 'x3', 1, 7, 5, 32, 68, 3, 1, 1, acc=True), f('128x64_260', 'x3', 1, 3, 5, 36, 260, 1),
                f('128x128_wo5', 'x3', 1, 13, 5, 128, 128, 1), f('128x128_wo13', 'x3', 1, 7, 13, 68, 68, 3, 1, 1), f('128x128_260', 'x3', 1, 1, 5, 260, 260, 3, 1, 1),
                f('chunked_13x13', 'x3', 4, 13, 13, 64, 64, 3, 1, 1), f('chunked_13x13_acc', 'x3', 5, 13, 13, 36, 68, 1, acc=True),
                f('slices', 'x3', 1, 5, 5, 32, 36, 3, 1, 1, inx=(8, 4), outx=(12, 8))]
    if cls == 'magic':                                           # divisors of 1 and powers of two in m / (Ho Wo) and r / Wo
        return [f('hw1_b3', 'x3', 3, 1, 1, 32, 32, 1), f('hw1_b40_k3', 'x3', 40, 1, 1, 36, 64, 3, 1, 1, positive=True), f('hw1_b64', 'x3', 64, 1, 1, 64, 68, 1),
                f('wo1_ho8', 'x3', 2, 8, 1, 32, 32, 3, 1, 1), f('wo2', 'x3', 3, 3, 2, 64, 32, 3, 1, 1), f('wo8_ho8', 'x3', 2, 8, 8, 32, 36, 3, 1, 1),
                f('wo16_s2', 'x3', 1, 6, 32, 36, 32, 3, 2, 1)]
    if cls == 'scales':                                          # 2^+-3 of head room on both operand scales; tiny and large gradients
        return [f('base', 'x3', 1, 6, 8, 64, 64, 3, 1, 1), f('base_up3', 'x3', 1, 6, 8, 64, 64, 3, 1, 1, shift=3),      # one set of operands (wgrad_make)
                f('base_down3', 'x3', 1, 6, 8, 64, 64, 3, 1, 1, shift=-3),
                f('gy_3e-7', 'x3', 1, 6, 8, 36, 68, 3, 1, 1, gymag=3e-7), f('gy_40', 'x3', 1, 6, 8, 36, 68, 3, 1, 1, gymag=40.0),
                f('gy_3e-7_up3', 'x3', 1, 2, 32, 64, 36, 1, shift=3, gymag=3e-7), f('gy_40_down3', 'x3', 1, 5, 5, 68, 32, 3, 1, 1, shift=-3, gymag=40.0),
                f('gy_40_up3_acc', 'x3', 2, 4, 4, 32, 32, 1, shift=3, gymag=40.0, acc=True), f('gy_3e-7_row32', 'x3', 1, 3, 32, 32, 32, 3, 1, 1, gymag=3e-7)]
    raise KeyError(cls)


def all_wgrad_cases():
    return [c for cls in WGRAD_CLASSES for v in WGRAD_VARIANTS for c in wgrad_cases(cls, v)]


def all_x3_cases():
    return [c for cls in X3_CLASSES for v in X3_VARIANTS for c in x3_cases(cls, v)]


# ----------------------------------------------------------------------------------------------------- restated launch plans
def wgrad_flat(c):
    return c.Cin < 16 and c.kh * c.kw > 1


def wgrad_vec4(c):
    return (c.Cin % 4 == 0 and c.Cout % 4 == 0 and c.in_cs % 4 == 0 and c.in_coff % 4 == 0 and c.out_cs % 4 == 0 and c.out_coff % 4 == 0
            and not c.misx and not c.misg)


def wgrad_plan(c):
    """dir_conv2d_wgrad_f32: (kernel, chunks, chunk length in pixels)"""
    M, t = c.B * c.Ho * c.Wo, lambda n: -(-n // 64)      # noqa: E731
    per = t(c.kh * c.kw * c.Cin) * t(c.Cout) if wgrad_flat(c) else t(c.Cin) * t(c.Cout) * c.kh * c.kw
    chunks = max(1, min(-(-1024 // per), -(-M // 256)))
    chunk = -(-(-(-M // chunks)) // 16) * 16
    if wgrad_flat(c):
        return 'conv_wgrad_flatk_kernel', chunks, chunk
    if wgrad_vec4(c):
        return 'conv_wgrad4_kernel', chunks, -(-chunk // 32) * 32
    return 'conv_wgrad_kernel', chunks, chunk


def wgrad_expected(c):
    k, chunks, _ = wgrad_plan(c)
    return [k] + (['wgrad_reduce_kernel'] if chunks > 1 or c.acc else [])


def wgrad_workspace_bytes(c):
    _, chunks, _ = wgrad_plan(c)
    return chunks * c.Cout * c.kh * c.kw * c.Cin * 4 if chunks > 1 else 0


def x3_tile(c):
    return (128 if c.Cout > 64 else 64, 128 if c.Cin > 64 else 64)


def x3_form(c):
    return 32 if c.Wo % 32 == 0 else 4 if c.Wo % 4 == 0 else 0


def x3_chunk_len(c, chunks):
    M = c.B * c.Ho * c.Wo
    return -(-(-(-M // chunks)) // 32) * 32


def x3_nominal_chunks(c):
    """the chunk count the CPU emulation is cut at (the device's own count follows its CU count and is read from the workspace size on the GPU)"""
    return max(1, min(-(-(c.B * c.Ho * c.Wo) // 512), 4))


# ----------------------------------------------------------------------------------------------------- operands and references
def pow2_in_scale(amax):
    """dir_amd.functional.pow2_in_scale on a known maximum"""
    import math
    return 2.0 ** (10 - math.frexp(float(amax))[1]) if amax > 0 and math.isfinite(amax) else 1.0


def activated(c, o, dtype):
    """the x operand the kernel multiplies: act(fma(x, ps, pb)) -- float32: one rounding of the fma, as the kernel's fmaf"""
    x = o['x'].astype(np.float64)
    if not c.pre:
        return x.astype(dtype)
    t = x * o['ps'].astype(np.float64) + o['pb'].astype(np.float64)
    t = t.astype(dtype)
    return np.maximum(t, 0) if c.pre == 'relu' else t


def wgrad_make(c):
    """-> dict: x [B, H, W, Cin], gy [B, Ho, Wo, Cout] (the owned channels), xbuf / gybuf (the NHWC buffers with NaN outside the slices), gw0 (the
    prefilled gradient, FILL without accumulate), ps / pb, sx / sg (x3)"""
    rng, span = _rng(c.name.replace('_up3', '').replace('_down3', '')), (X3_SPAN if c.api == 'x3' else 8.0)      # (a shifted case: its base's operands)
    x = _vals(rng, c.B * c.H * c.W * c.Cin, c.positive, span).reshape(c.B, c.H, c.W, c.Cin)
    gy = (_vals(rng, c.B * c.Ho * c.Wo * c.Cout, c.positive, span).astype(np.float64) * c.gymag).astype(F).reshape(c.B, c.Ho, c.Wo, c.Cout)
    o = dict(x=x, gy=gy, ps=None, pb=None)
    if c.pre:
        ch = np.arange(c.Cin)
        ps = (2.0 ** rng.randint(-2, 3, c.Cin) * (1.0 + 0.25 * rng.rand(c.Cin)) * np.where(ch % 3 == 1, -1.0, 1.0)).astype(F)     # negative on a third
        pb = (0.5 + rng.rand(c.Cin) * 4.0).astype(F)                                         # > 0 on every channel (but the dead ones below)
        # t = x ps + pb = pb (1 + q): q in +-[2, 32] or +-[1/32, 1/2], so 0.25 <= pb / 2 <= |t| <= 33 pb whatever the signs (no cancellation into
        # the f16 denormals, see X3_SPAN), both signs of t on every channel
        q = 2.0 ** rng.uniform(1.0, 5.0, x.shape) * rng.choice((-1.0, 1.0), x.shape)
        q = np.where(rng.rand(*x.shape) < 0.5, q, 1.0 / q)
        o['x'] = x = (q * pb.astype(np.float64) / ps.astype(np.float64)).astype(F)
        dead = ch % 7 == 3                                                                     # channels whose activation is all zero
        ps[dead], pb[dead] = (-1.0, -(float(np.abs(x).max()) + 1.0)) if c.pre == 'relu' else (0.0, 0.0)
        if c.pre == 'relu':
            x[..., dead] = np.abs(x[..., dead])
        o.update(ps=ps, pb=pb)
    xb = np.full((c.B, c.H, c.W, c.in_cs), np.nan, F)
    xb[..., c.in_coff:c.in_coff + c.Cin] = x
    gb = np.full((c.B, c.Ho, c.Wo, c.out_cs), np.nan, F)
    gb[..., c.out_coff:c.out_coff + c.Cout] = gy
    o.update(xbuf=xb, gybuf=gb, gw0=_vals(rng, c.Cout * c.kh * c.kw * c.Cin).reshape(c.Cout, c.kh, c.kw, c.Cin) if c.acc else None)
    if c.api == 'x3':
        o.update(sx=pow2_in_scale(np.abs(activated(c, o, F)).max()) * 2.0 ** c.shift, sg=pow2_in_scale(np.abs(gy).max()) * 2.0 ** c.shift)
    return o


def im2col(c, xa):
    """xa [B, H, W, Cin] -> (X [M, taps, Cin] with zeros in the padding, inside [M, taps] bool)"""
    s, p = c.stride, c.pad
    xp = np.zeros((c.B, c.H + 2 * p + s * c.Ho + c.kh, c.W + 2 * p + s * c.Wo + c.kw, c.Cin), xa.dtype)
    ins = np.zeros(xp.shape[:3], bool)
    xp[:, p:p + c.H, p:p + c.W] = xa
    ins[:, p:p + c.H, p:p + c.W] = True
    X = np.empty((c.B, c.Ho, c.Wo, c.kh * c.kw, c.Cin), xa.dtype)
    I = np.empty((c.B, c.Ho, c.Wo, c.kh * c.kw), bool)
    for ky in range(c.kh):
        for kx in range(c.kw):
            X[:, :, :, ky * c.kw + kx] = xp[:, ky:ky + s * c.Ho:s, kx:kx + s * c.Wo:s][:, :c.Ho, :c.Wo]
            I[:, :, :, ky * c.kw + kx] = ins[:, ky:ky + s * c.Ho:s, kx:kx + s * c.Wo:s][:, :c.Ho, :c.Wo]
    M = c.B * c.Ho * c.Wo
    return X.reshape(M, c.kh * c.kw, c.Cin), I.reshape(M, c.kh * c.kw)


def wgrad_reference(c, o, X=None, gy=None):
    """float64: (ref, S, terms) as [Cout, kh, kw, Cin]; terms: the in-image pixels of the element's tap"""
    Xi, inside = im2col(c, activated(c, o, np.float64))
    X = Xi if X is None else X
    M = X.shape[0]
    g = (o['gy'] if gy is None else gy).reshape(M, c.Cout).astype(np.float64)
    shape = (c.Cout, c.kh, c.kw, c.Cin)
    ref, S = (g.T @ X.reshape(M, -1)).reshape(shape), (np.abs(g).T @ np.abs(Xi).reshape(M, -1)).reshape(shape)
    if c.acc:
        ref, S = ref + o['gw0'].astype(np.float64), S + np.abs(o['gw0'].astype(np.float64))
    terms = np.broadcast_to(inside.sum(0).reshape(1, c.kh, c.kw, 1), shape)
    return ref, S, terms


def wgrad_float32(c, o, how, chunks=None, chunk=None):
    """dir_conv2d_wgrad_f32 in float32 on the CPU, cut at the restated chunk length, partials added in chunk order onto gw0 (or onto 0)"""
    if chunk is None:
        _, chunks, chunk = wgrad_plan(c)
    X, _ = im2col(c, activated(c, o, F))
    M = X.shape[0]
    g, X = o['gy'].reshape(M, c.Cout), X.reshape(M, -1)
    summer = sum_serial if how == 'serial' else sum_pairwise
    s = o['gw0'].reshape(c.Cout, -1).copy() if c.acc else np.zeros((c.Cout, X.shape[1]), F)
    for i in range(chunks):
        s = s + summer(g[i * chunk:(i + 1) * chunk], X[i * chunk:(i + 1) * chunk])
    return s.reshape(c.Cout, c.kh, c.kw, c.Cin)


def split_f16(v, s):
    """conv_common.h's split_f16x3: clamp(v s) = hi + lo in float16 (returned as float32: every f16 x f16 product is then exact)"""
    t = np.clip(v.astype(F) * F(s), -F16_MAX, F16_MAX).astype(F)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(F)).astype(np.float16)
    return hi.astype(F), lo.astype(F)


def x3_emulate(c, o, chunks=None):
    """the split arithmetic on the CPU: per chunk hi hi + lo hi + hi lo with float32 accumulation (pairwise), x 1 / (sx sg); partials added in
    chunk order onto gw0"""
    chunks = x3_nominal_chunks(c) if chunks is None else chunks
    chunk = x3_chunk_len(c, chunks)
    X, _ = im2col(c, activated(c, o, F))
    M = X.shape[0]
    gh, gl = split_f16(o['gy'].reshape(M, c.Cout), o['sg'])
    xh, xl = split_f16(X.reshape(M, -1), o['sx'])
    inv = F(1.0 / (o['sx'] * o['sg']))
    s = o['gw0'].reshape(c.Cout, -1).copy() if c.acc else np.zeros((c.Cout, xh.shape[1]), F)
    for i in range(chunks):
        k = slice(i * chunk, (i + 1) * chunk)
        s = s + ((sum_pairwise(gh[k], xh[k]) + sum_pairwise(gl[k], xh[k])) + sum_pairwise(gh[k], xl[k])) * inv
    return s.reshape(c.Cout, c.kh, c.kw, c.Cin)
