"""tests/helpers/matmul_cases.py proved on the CPU: the case counts, the float64 references against independent ones (pointer arithmetic straight
from the descriptor for the GEMMs, torch's float64 autograd through conv2d for the weight gradients), the constants re-derived from the two float32
references (and the f16 split emulation) as the helper states them, the restated launch plans at the values the issue names, and check() rejecting
every mutant of the float64 reference it is meant to catch.  A mutant is a wrong ARRAY handed to the checker; no kernel runs here."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import matmul_cases as MC  # noqa: E402


@functools.lru_cache(maxsize=None)
def gemm_all():
    out = []
    for c in MC.all_gemm_cases():
        o = MC.gemm_make(c)
        out.append((c, o) + MC.gemm_reference(c, o))
    return out


@functools.lru_cache(maxsize=None)
def wgrad_all(api):
    out = []
    for c in (MC.all_wgrad_cases() if api == 'f32' else MC.all_x3_cases()):
        o = MC.wgrad_make(c)
        out.append((c, o) + MC.wgrad_reference(c, o))
    return out


def rejected(got, ref, S, kind, terms):
    try:
        MC.check(got, ref, S, kind, terms)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------ the lists
def test_case_counts_and_names():
    for cls in MC.GEMM_CLASSES:
        for t in MC.TA_TB:
            assert len(MC.gemm_cases(cls, t)) == MC.GEMM_COUNTS[cls], cls
    for cls in MC.WGRAD_CLASSES:
        for v in MC.WGRAD_VARIANTS:
            assert len(MC.wgrad_cases(cls, v)) == MC.WGRAD_COUNTS[cls], cls
    for cls in MC.X3_CLASSES:
        for v in MC.X3_VARIANTS:
            assert len(MC.x3_cases(cls, v)) == MC.X3_COUNTS[cls], cls
    for cases in (MC.gemm_cases('tails', (0, 0)) + MC.gemm_cases('grouped', (1, 0)), MC.wgrad_cases('chunks', 'write'), MC.x3_cases('row0', 'relu')):
        assert len({c.name for c in cases}) == len(cases)


def test_the_edges_the_issue_names_are_in_the_lists():
    tails = MC.gemm_cases('tails', (0, 0))
    assert {c.M for c in tails} >= set(MC.MN_VALUES) and {c.N for c in tails} >= set(MC.MN_VALUES) and {c.K for c in tails} == set(MC.K_VALUES)
    grid = {-(-c.M // 64) * -(-c.N // 64) * c.batch for c in MC.gemm_cases('grid', (0, 0))}
    assert {128, 129} <= grid
    st = MC.gemm_cases('strides', (0, 0))
    assert any(c.pa and c.pb and c.pc for c in st) and {1, 2, 4} <= {c.mis for c in st} and any(c.sb0 for c in st) and any(c.gapc for c in st)
    assert {(c.bias, c.acc) for c in st} == {(False, False), (True, False), (False, True), (True, True)}
    gr = MC.gemm_cases('grouped', (0, 0))
    assert {(c.ny, c.nx) for c in gr} == {(1, 1), (1, 3), (3, 3)} and {1, 2} <= {c.neg for c in gr}
    assert all({(c.M, r) for c in gr for r in (c.reduce,)} >= {(M, r)} for M in (65, 79, 80) for r in (0, 1))
    assert any(c.reduce and c.K % 32 and c.bias and c.acc for c in gr)
    sk = MC.gemm_cases('splitk', (0, 0))
    assert {c.K for c in sk} >= set(MC.SPLITK_K) and any(c.K == 64 * 129 and c.M <= 64 and c.N <= 64 for c in sk)
    assert any(c.bias for c in sk) and any(c.acc for c in sk) and any(c.pc for c in sk)
    x3 = MC.all_x3_cases()
    assert {c.Cin for c in x3} | {c.Cout for c in x3} == {32, 36, 64, 68, 128, 132, 260}
    assert {c.Wo for c in x3 if c.cls in ('row4', 'row0')} >= {4, 12, 1, 5, 13}
    assert any(c.B * c.Ho * c.Wo < 32 for c in x3) and any(c.B * c.Ho * c.Wo == 32 for c in x3) and any(c.B * c.Ho * c.Wo == 96 for c in x3)
    assert any(c.Ho * c.Wo == 1 for c in x3) and any(c.Wo == 1 and c.Ho > 1 for c in x3) and {-3, 3} <= {c.shift for c in x3}


def test_every_kernel_and_form_serves_three_cases_of_its_class():
    for cls in MC.GEMM_CLASSES:
        for t in MC.TA_TB:
            names = [k for c in MC.gemm_cases(cls, t) for k in MC.gemm_expected(c)]
            for k in MC.GEMM_EXPECTED[cls]:
                assert names.count(k) >= 3, (cls, t, k)
    for cls in MC.WGRAD_CLASSES:
        for v in MC.WGRAD_VARIANTS:
            names = [k for c in MC.wgrad_cases(cls, v) for k in MC.wgrad_expected(c)]
            for k in MC.WGRAD_EXPECTED[cls]:
                assert names.count(k) >= 3, (cls, v, k)
    for cls, form in MC.X3_FORMS.items():
        for v in MC.X3_VARIANTS:
            seen = [(MC.x3_tile(c), MC.x3_form(c)) for c in MC.x3_cases(cls, v)]
            for tile in MC.X3_TILES:
                assert seen.count((tile, form)) >= 3, (cls, v, tile)


def test_restated_wgrad_plan_at_the_named_values():
    by = {c.name: c for c in MC.wgrad_cases('chunks', 'write') + MC.wgrad_cases('dispatch', 'write')}
    c = by['chunks-empty_last_chunk']
    kernel, chunks, chunk = MC.wgrad_plan(c)
    M = c.B * c.Ho * c.Wo
    assert (kernel, chunks, chunk, M) == ('conv_wgrad4_kernel', 15, 288, 3850) and (chunks - 1) * chunk == 4032 > M > (chunks - 2) * chunk
    assert MC.wgrad_plan(by['chunks-odd_steps_k3']) == ('conv_wgrad4_kernel', 2, 256)             # 480 pixels: 8 steps | 7 steps
    for M, chunks in ((255, 1), (256, 1), (257, 2), (513, 3)):
        assert MC.wgrad_plan(by['chunks-vector_M%d' % M])[:2] == ('conv_wgrad4_kernel', chunks)
        assert MC.wgrad_plan(by['chunks-scalar_M%d' % M])[:2] == ('conv_wgrad_kernel', chunks)
        assert MC.wgrad_plan(by['chunks-flat_M%d' % M])[:2] == ('conv_wgrad_flatk_kernel', chunks)
    assert MC.wgrad_plan(by['chunks-vector_M257'])[2] == 160 and MC.wgrad_plan(by['chunks-scalar_M257'])[2] == 144     # 32- and 16-pixel rounding
    assert MC.wgrad_plan(by['dispatch-flat_stem'])[0] == MC.wgrad_plan(by['dispatch-flat_cin15'])[0] == 'conv_wgrad_flatk_kernel'
    assert MC.wgrad_plan(by['dispatch-scalar_cin15_k1'])[0] == 'conv_wgrad_kernel' and MC.wgrad_plan(by['dispatch-vector_cin16_k3'])[0] == 'conv_wgrad4_kernel'
    for n in ('scalar_cin18', 'scalar_cout6', 'scalar_coff2', 'scalar_misx', 'scalar_misg'):
        assert MC.wgrad_plan(by['dispatch-' + n])[0] == 'conv_wgrad_kernel', n


def test_gemm_expected_kernels_at_the_grid_boundary():
    by = {c.name: c for c in MC.gemm_cases('grid', (0, 0)) + MC.gemm_cases('splitk', (0, 0)) + MC.gemm_cases('grouped', (0, 0))}
    assert MC.gemm_expected(by['grid-M64_N64_b128_t00']) == ['gemm_f32_small_kernel'] and MC.gemm_expected(by['grid-M64_N64_b129_t00']) == ['gemm_f32_kernel']
    assert MC.gemm_expected(by['grid-M65_N65_b32_t00']) == ['gemm_f32_small_kernel'] and MC.gemm_expected(by['grid-M65_N65_b33_t00']) == ['gemm_f32_kernel']
    assert MC.gemm_expected(by['splitk-K8256_small_grid_t00'])[0] == 'gemm_f32_small_kernel' and MC.gemm_expected(by['splitk-K8256_t00'])[0] == 'gemm_f32_kernel'
    for M, k in ((64, 'gemm_f32_grouped_kernel'), (65, 'gemm_f32_grouped_short_kernel'), (80, 'gemm_f32_grouped_short_kernel'), (81, 'gemm_f32_grouped_kernel')):
        assert MC.gemm_expected(by['grouped-M%d_r0_t00' % M]) == [k]


# ------------------------------------------------------------------------------------------------------------------ operands and references
def test_gemm_operands_own_what_they_index_and_nothing_else():
    for c, o, ref, S, _ in gemm_all():
        assert np.isfinite(o['A']).all() and np.isfinite(o['B']).all() and np.isfinite(ref).all() and (S >= 0).all(), c.name
        L = o['L']
        for buf, idx in ((o['a'], L.idxA), (o['b'], L.idxB)):
            own = np.zeros(buf.size, bool)
            own[idx.ravel()] = True
            assert np.isnan(buf[~own]).all()
        if c.pa:
            assert np.isnan(o['a'][L.idxA[0, 0, c.M - 1, c.K - 1] + 1])
        if c.gapa and c.batch > 1 and c.nx * c.ny == 1:
            assert np.isnan(o['a'][L.idxA[0].max() + 1])
        if c.rowscale:
            amax = np.abs(o['A'][0, 0]).max(1)
            assert amax.max() / amax.min() > 1e8


def test_gemm_reference_against_pointer_arithmetic():
    """C[b][g][m][n] from the flat buffers with the addresses written out as the header states them (no index arrays)"""
    for c, o, ref, S, _ in gemm_all():
        L, a, b = o['L'], o['a'].astype(np.float64), o['b'].astype(np.float64)
        ng = c.ny * c.nx
        for bz in {0, c.batch - 1}:
            for m, n in {(0, 0), (c.M - 1, c.N - 1), (c.M // 2, c.N // 3)}:
                tot = np.zeros(ng)
                for g in range(ng):
                    gy, gx = divmod(g, c.nx)
                    pa, pb = L.a0 + bz * L.sA + gy * L.a_y + gx * L.a_x, L.b0 + bz * L.sB + gy * L.b_y + gx * L.b_x
                    k = np.arange(c.K)
                    av = a[pa + (k * L.lda + m if c.ta else m * L.lda + k)]
                    bv = b[pb + (n * L.ldb + k if c.tb else k * L.ldb + n)]
                    tot[g] = float(np.dot(av, bv))
                extra = (float(o['bias'][n]) if c.bias else 0.0)
                if c.api == 'grouped' and not c.reduce:
                    for g in range(ng):
                        gy, gx = divmod(g, c.nx)
                        pc = bz * L.sC + gy * L.c_y + gx * L.c_x + m * L.ldc + n
                        assert L.idxC[bz, g, m, n] == pc
                        want = tot[g] + extra + (float(o['c0'][pc]) if c.acc else 0.0)
                        assert abs(ref[bz, g, m, n] - want) <= 1e-12 * S[bz, g, m, n], c.name
                else:
                    pc = bz * L.sC + m * L.ldc + n
                    assert L.idxC[bz, 0, m, n] == pc
                    want = tot.sum() + extra + (float(o['c0'][pc]) if c.acc else 0.0)
                    assert abs(ref[bz, 0, m, n] - want) <= 1e-12 * S[bz, 0, m, n], c.name


@pytest.mark.parametrize('api', ['f32', 'x3'])
def test_wgrad_reference_against_torch_autograd(api):
    for c, o, ref, S, terms in wgrad_all(api):
        xa = torch.from_numpy(MC.activated(c, o, np.float64).transpose(0, 3, 1, 2).copy())
        w = torch.zeros(c.Cout, c.Cin, c.kh, c.kw, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(xa, w, stride=c.stride, padding=c.pad)
        assert y.shape[2] >= c.Ho and y.shape[3] >= c.Wo, c.name
        (y[:, :, :c.Ho, :c.Wo] * torch.from_numpy(o['gy'].astype(np.float64).transpose(0, 3, 1, 2).copy())).sum().backward()
        want = w.grad.permute(0, 2, 3, 1).numpy() + (o['gw0'].astype(np.float64) if c.acc else 0.0)
        assert (np.abs(ref - want) <= 1e-11 * S + 1e-300).all(), c.name
        assert ((S == 0) == (np.broadcast_to(terms, S.shape) == 0)).all() or c.pre or c.acc, c.name        # no in-image pixel <=> S = 0
        assert np.isnan(o['xbuf']).sum() == c.B * c.H * c.W * (c.in_cs - c.Cin) and np.isnan(o['gybuf']).sum() == c.B * c.Ho * c.Wo * (c.out_cs - c.Cout)


def test_exact_zero_taps_exist_and_are_positive_elsewhere():
    n = 0
    for c, o, ref, S, terms in wgrad_all('f32') + wgrad_all('x3'):
        if c.positive:
            zero = np.broadcast_to(terms, S.shape) == 0
            base = o['gw0'].astype(np.float64) if c.acc else np.zeros(S.shape)
            assert zero.any() and (ref[zero] == base[zero]).all() and (S[zero] == np.abs(base[zero])).all(), c.name
            if not c.pre:
                assert ((ref - base)[~zero] > 0).all(), c.name
            n += 1
    assert n >= 10


def test_shifted_scales_share_their_base_operands():
    by = {c.name: MC.wgrad_make(c) for c in MC.x3_cases('scales', 'relu')}
    base = by['scales-base']
    for n, k in (('scales-base_up3', 8.0), ('scales-base_down3', 0.125)):
        o = by[n]
        assert np.array_equal(o['x'], base['x']) and np.array_equal(o['gy'], base['gy']) and o['sx'] == k * base['sx'] and o['sg'] == k * base['sg']
    assert 1e-7 < np.abs(by['scales-gy_3e-7']['gy']).max() < 2e-5 and 40.0 < np.abs(by['scales-gy_40']['gy']).max() < 40.0 * 64


def test_x3_operands_stay_inside_the_split_guarantee():
    """scaled operands in [2^-3 x 2/3, 65504) or exactly 0 (matmul_cases' docstring), scales powers of two; dead channels are all zero"""
    for c, o, _, _, _ in wgrad_all('x3'):
        xa, g = np.abs(MC.activated(c, o, np.float32)).astype(np.float64) * o['sx'], np.abs(o['gy']).astype(np.float64) * o['sg']
        for v in (xa, g):
            assert v.max() < MC.F16_MAX and v[v > 0].min() >= 2.0 ** -3 * 2 / 3, c.name
        assert 2.0 ** (6 if c.shift < 0 else 9) <= xa.max() and np.log2(o['sx']) % 1 == 0 and np.log2(o['sg']) % 1 == 0
        if c.pre:
            assert (o['pb'][np.arange(c.Cin) % 7 != 3] > 0).all() and (o['ps'] < 0).any()
            assert (xa[..., np.arange(c.Cin) % 7 == 3] == 0).all()
            t = o['x'].astype(np.float64) * o['ps'] + o['pb']
            assert (t < 0).any() and (t > 0).any()


# ------------------------------------------------------------------------------------------------------------------ the constants
def _pin(kind, measured):
    assert abs(measured - MC.RATIOS[kind]) <= 0.01 * MC.RATIOS[kind], '%s: measured %.4f, recorded %.4f' % (kind, measured, MC.RATIOS[kind])
    assert MC.C[kind] == 4.0 * MC.RATIOS[kind]


def test_constants_are_derived_from_the_float32_references():
    """RATIOS[kind] = the larger of the serial and the pairwise float32 reference's distance from float64 over the list; every float32 serial
    reference passes check() (so no case cancels so hard that S means nothing)"""
    worst = {k: [0.0, 0.0] for k in ('gemm', 'splitk', 'wgrad')}
    for c, o, ref, S, terms in gemm_all():
        kind = 'splitk' if c.api == 'splitk' else 'gemm'
        for i, how in enumerate(('serial', 'pairwise')):
            got = MC.gemm_float32(c, o, how)
            worst[kind][i] = max(worst[kind][i], MC.ratio(got, ref, S))
            if how == 'serial':
                MC.check(got, ref, S, kind, terms, c.name)
    for c, o, ref, S, terms in wgrad_all('f32'):
        for i, how in enumerate(('serial', 'pairwise')):
            got = MC.wgrad_float32(c, o, how)
            worst['wgrad'][i] = max(worst['wgrad'][i], MC.ratio(got, ref, S))
            if how == 'serial':
                MC.check(got, ref, S, 'wgrad', terms, c.name)
    print('MATMUL-RATIOS (serial, pairwise): %s' % {k: tuple(round(x, 4) for x in v) for k, v in worst.items()})
    for kind, v in worst.items():
        _pin(kind, max(v))


def test_x3_constant_is_the_emulation_plus_the_float32_reference():
    emu = f32 = 0.0
    for c, o, ref, S, terms in wgrad_all('x3'):
        n = MC.x3_nominal_chunks(c)
        L = MC.x3_chunk_len(c, n)
        e = MC.x3_emulate(c, o)
        emu = max(emu, MC.ratio(e, ref, S))
        for how in ('serial', 'pairwise'):
            got = MC.wgrad_float32(c, o, how, n, L)
            f32 = max(f32, MC.ratio(got, ref, S))
            MC.check(got, ref, S, 'x3', terms, c.name)
        MC.check(e, ref, S, 'x3', terms, c.name)                 # the arithmetic itself fits the 2^-20 S cap on these operands
    print('MATMUL-RATIOS x3: emulation %.4f + float32 reference %.4f' % (emu, f32))
    _pin('x3', emu + f32)
    assert float(MC.c_eff('x3', 1)) == min(MC.C['x3'], MC.X3_CAP) == 16.0


def test_bound_form():
    assert float(MC.c_eff('gemm', 1)) == 3.0 and float(MC.c_eff('gemm', 10 ** 6)) == MC.C['gemm']
    assert MC.tol(0.0, 'wgrad', 5) == MC.FLOOR == np.float64(np.finfo(np.float32).smallest_subnormal)
    assert MC.check(np.zeros(3), np.zeros(3), np.zeros(3), 'wgrad', 0) == 0.0
    assert rejected(np.array([2.0 ** -148]), np.zeros(1), np.zeros(1), 'wgrad', 0)                # S = 0: only 0 (or one denormal) passes
    assert rejected(np.array([np.nan]), np.ones(1), np.ones(1), 'gemm', 9) and rejected(np.array([np.inf]), np.ones(1), np.ones(1), 'gemm', 9)
    assert not rejected(np.array([1.0 + 3 * MC.U]), np.ones(1), np.ones(1), 'gemm', 1) and rejected(np.array([1.0 + 3.1 * MC.U]), np.ones(1), np.ones(1), 'gemm', 1)


# ------------------------------------------------------------------------------------------------------------------ mutants
def _gemm_mutants(cls, pick, mutate, kind=None):
    hit = tried = 0
    for c, o, ref, S, terms in gemm_all():
        if c.cls == cls and pick(c):
            tried += 1
            hit += rejected(mutate(c, o, ref), ref, S, kind or ('splitk' if c.api == 'splitk' else 'gemm'), terms)
    assert tried and hit, (cls, tried, hit)
    return hit, tried


def test_mutant_last_k_term_dropped():
    def m(c, o, ref):
        A = o['A'].copy()
        A[..., c.K - 1] = 0
        return MC.gemm_reference(c, o, A=A)[0]
    hit, tried = _gemm_mutants('tails', lambda c: True, m)
    assert hit == tried                                          # every case: one term of K is far above c 2^-24 S
    _gemm_mutants('splitk', lambda c: True, m)


def test_mutant_k_term_counted_twice_at_a_step_boundary():
    m = lambda c, o, ref: ref + np.matmul(o['A'][..., 32:33].astype(np.float64), o['B'][..., 32:33, :].astype(np.float64))      # noqa: E731
    for cls in ('tails', 'splitk'):
        _gemm_mutants(cls, lambda c: c.K > 32, m)


def test_mutant_last_row_is_the_row_before():
    def m(c, o, ref):
        got = ref.copy()
        got[..., c.M - 1, :] = got[..., c.M - 2, :]
        return got
    for cls in ('tails', 'rowscale', 'grouped'):
        _gemm_mutants(cls, lambda c: c.M > 1, m)


def test_mutant_pad_column_of_a_read_for_a_tail_element():
    def m(c, o, ref):
        A = o['A'].copy()
        A[..., c.M - 1, c.K - 1] = o['a'][o['L'].idxA[..., c.M - 1, c.K - 1] + 1]
        return MC.gemm_reference(c, o, A=A)[0]
    hit, tried = _gemm_mutants('strides', lambda c: c.pa > 0, m)
    assert hit == tried


def test_mutant_bias_added_twice_under_accumulate():
    m = lambda c, o, ref: MC.gemm_reference(c, o, bias_times=2)[0]      # noqa: E731
    for cls in ('strides', 'grouped', 'splitk'):
        _gemm_mutants(cls, lambda c: c.bias and c.acc, m)


def test_mutant_one_group_displaced_by_one_element():
    def m(c, o, ref):
        L = o['L']
        idx = L.idxA.copy()
        idx[:, 1] = np.minimum(idx[:, 1] + 1, L.nA - 1)
        return MC.gemm_reference(c, o, A=o['a'][idx])[0]
    hit, tried = _gemm_mutants('grouped', lambda c: c.ny * c.nx > 1, m)
    assert hit == tried


def _wgrad_mutants(api, pick, mutate):
    hit = tried = 0
    for c, o, ref, S, terms in wgrad_all(api):
        if pick(c):
            tried += 1
            hit += rejected(mutate(c, o, ref), ref, S, 'wgrad' if api == 'f32' else 'x3', terms)
    assert tried and hit == tried, (tried, hit)


def _gx(c, o):
    X, inside = MC.im2col(c, MC.activated(c, o, np.float64))
    M = X.shape[0]
    return o['gy'].reshape(M, c.Cout).astype(np.float64), X, inside


def test_mutant_padding_tap_picks_up_the_activated_shift():
    """a kernel that masked before activating: every padding pixel of a tap adds relu(pre_shift[ci]) gy[m][co]"""
    def m(c, o, ref):
        g, X, inside = _gx(c, o)
        got = ref.copy()
        got[:, 0, 0, :] += np.outer(g[~inside[:, 0]].sum(0), np.maximum(o['pb'].astype(np.float64), 0.0))
        return got
    _wgrad_mutants('x3', lambda c: c.pre == 'relu' and c.pad == 1 and c.kh == 3 and c.kw == 3, m)


def test_mutant_pixel_at_a_chunk_boundary_counted_twice():
    def m(c, o, ref):
        g, X, _ = _gx(c, o)
        k = MC.wgrad_plan(c)[2]
        return ref + np.outer(g[k], X[k].reshape(-1)).reshape(ref.shape)
    _wgrad_mutants('f32', lambda c: c.cls == 'chunks' and MC.wgrad_plan(c)[1] > 1, m)


def test_mutant_empty_chunk_repeats_the_last_step():
    def m(c, o, ref):
        g, X, _ = _gx(c, o)
        _, chunks, chunk = MC.wgrad_plan(c)
        M, beg = X.shape[0], (chunks - 2) * chunk
        m0 = beg + (M - 1 - beg) // 32 * 32
        return ref + (g[m0:M].T @ X[m0:M].reshape(M - m0, -1)).reshape(ref.shape)
    _wgrad_mutants('f32', lambda c: c.name == 'chunks-empty_last_chunk', m)


def test_mutant_image_index_off_by_one_on_a_one_pixel_map():
    def m(c, o, ref):
        X, _ = MC.im2col(c, np.roll(MC.activated(c, o, np.float64), -1, axis=0))
        return MC.wgrad_reference(c, o, X=X)[0]
    _wgrad_mutants('x3', lambda c: c.cls == 'magic' and c.Ho * c.Wo == 1, m)
