"""The norm sweep's helper (tests/helpers/norm_cases.py) on the CPU: the case lists are what the sweep is meant to run and select every kernel it
names; the float64 references agree with torch's float64 autograd; both float32 references (torch's own CPU operator, a numpy evaluation in the
kernels' documented order) stay inside the per-element bound at c / 4; the operands have the stated structure; the check, with the constants the
GPU run uses, rejects fourteen single defects on every case they change; a last test shows which of them the max-norm gates of the existing parity
tests let through on those tests' own data."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import norm_cases as NC  # noqa: E402

_CACHE = {}


def bn_operands(case, variant):
    """operands of one case, made once and shared (read-only) by the tests of this module"""
    key = (case.name, variant)
    if key not in _CACHE:
        _CACHE[key] = NC.bn_make(case, variant)
    return _CACHE[key]


def survey():
    """both float32 references judged on every case, once: -> {'np' | 'torch': Tally}, the largest undecided band"""
    if 'survey' in _CACHE:
        return _CACHE['survey']
    n_threads = torch.get_num_threads()
    torch.set_num_threads(NC.TORCH_THREADS)                           # torch's reductions in one fixed order
    saved = dict(NC.C)
    try:
        tot = {'np': NC.Tally(), 'np_capped': NC.Tally(), 'torch': NC.Tally()}
        for case in NC.bn_cases():
            for v in NC.BN_VARIANTS:
                o = bn_operands(case, v)
                tot['np_capped'].merge(NC.bn_judge(case, v, o, NC.bn_standin32(case, v, o)))
                if case.api in ('train', 'split') and case.R > 1:
                    tot['torch'].merge(NC.bn_judge(case, v, o, NC.bn_standin_torch(case, v, o)))
        for case in NC.ln_cases():
            o = NC.ln_make(case)
            for m in NC.LN_MODES:
                tot['np_capped'].merge(NC.ln_judge(case, o, NC.ln_standin(case, o, m), m))
                if case.C > 1:                                        # (one column: torch's weight gradient is 49 where the exact one is 0)
                    tot['torch'].merge(NC.ln_judge(case, o, NC.ln_standin(case, o, m, torch32=True), m))
        for case in NC.att_cases():
            o = NC.att_make(case)
            tot['np_capped'].merge(NC.att_judge(case, o, NC.att_standin(case, o)))
            tot['torch'].merge(NC.att_judge(case, o, NC.att_standin(case, o, torch32=True)))
        for case in NC.gelu_cases():
            o = NC.gelu_make(case)
            tot['np_capped'].merge(NC.gelu_judge(case, o, NC.gelu32(o)))
            tot['torch'].merge(NC.gelu_judge(case, o, NC.gelu_torch32(o)))
        for case in NC.colsum_cases():
            o = NC.colsum_make(case)
            for a in (False, True):
                tot['np_capped'].merge(NC.colsum_judge(case, o, NC.colsum32(o, a), a))
    finally:
        torch.set_num_threads(n_threads)
        NC.C.update(saved)
    _CACHE['survey'] = tot
    return tot


# ------------------------------------------------------------------------------------------------------------------------------ the lists
def test_case_lists_are_what_the_sweep_is_meant_to_run():
    L = NC.bn_cases()
    assert L == NC.bn_cases() and len({c.name for c in L}) == len(L)                         # deterministic, named
    assert NC.ln_cases() == NC.ln_cases() and NC.att_cases() == NC.att_cases() and NC.colsum_cases() == NC.colsum_cases()
    by = lambda cls: NC.bn_cases(cls)      # noqa: E731
    assert all(len(by(cls)) >= 3 for cls in NC.BN_CLASSES)
    assert all(c.R * c.ld <= 1200000 and c.C in NC.BN_CHANNELS for c in L)
    assert {c.R for c in by('small')} >= {1, 2, 15} and any(c.C == 260 for c in by('small')) and any(c.C % 4 and c.R > 15 for c in by('small'))
    assert {(c.R, c.C) for c in by('mid')} == {(R, Cn) for R in NC.MID_R for Cn in (4, 8, 20, 36, 68, 132)}
    assert {(c.R, c.C) for c in by('chunk_vec')} == {(R, Cn) for R in NC.CHUNK_R for Cn in (4, 60, 64, 68, 132)}
    assert {c.R - 512 for c in by('chunk_vec')} >= {1, 16, 17, 49, 65, 255, 256} and {-(-c.R // 256) for c in by('chunk_vec')} >= {16, 17, 18, 33}
    assert {(c.R, c.C) for c in by('chunk_scalar') if not c.mis} == {(R, Cn) for R in NC.CHUNK_R for Cn in (3, 6)}
    assert sum(c.mis and c.C == 8 for c in by('chunk_scalar')) >= 3
    for path in ('small', 'mid', 'chunk_vec'):
        assert any(c.ld == c.C + 4 and NC.bn_path(c) == path for c in by('strided')), path
    assert {NC.bn_path(c) for c in by('strided') if c.ld == c.C + 1} == {'small', 'chunk_scalar'}
    assert all(NC.bn_path(c) == 'chunk_vec' for c in by('split')) and {NC.bn_path(c) for c in by('frozen')} >= {'mid', 'chunk_vec'}
    chunks = lambda c: -(-c.R // c.chunk_rows)      # noqa: E731
    assert {(c.chunk_rows, chunks(c)) for c in by('partials')} == {(r, k) for r in (8, 64) for k in (255, 256, 257)}
    assert any(c.R % c.chunk_rows for c in by('partials')) and any(c.cap == chunks(c) == 257 for c in by('partials'))
    assert {len(c.splits) for c in by('sync')} == {1, 2, 3, 8} and all(sum(c.splits) == c.R for c in by('sync'))
    assert all(1 in c.splits and len(set(c.splits)) == len(c.splits) for c in by('sync') if len(c.splits) > 1)
    # the class of a case is the path the restated dispatch predicates select for it
    for c in L:
        if c.cls in ('small', 'mid', 'chunk_vec', 'chunk_scalar'):
            assert NC.bn_path(c) == c.cls, c.name
    assert {(c.R, c.C) for c in NC.ln_cases()} == {(R, Cn) for R in NC.LN_R for Cn in NC.LN_C} and {c.eps for c in NC.ln_cases()} == {1e-6, 1e-5}
    assert {(c.kind, c.T, c.H, c.B) for c in NC.att_cases()} == {(k, T, H, B) for k in NC.ATT_KINDS for T in NC.ATT_T for H in NC.ATT_H for B in NC.ATT_B}
    assert {c.n for c in NC.gelu_cases()} >= {1, 255, 256, 257, 1 << 16}
    assert {c.R for c in NC.colsum_cases()} >= {127, 128, 129, 511, 512, 513, 4095, 4096, 4097} and any(c.ld > c.N for c in NC.colsum_cases())


def test_dispatch_predicates_and_every_named_kernel_has_three_cases():
    assert NC.bn_vec4(8, 8, True) and not NC.bn_vec4(6, 6, True) and not NC.bn_vec4(8, 9, True) and not NC.bn_vec4(8, 8, False)
    K = lambda **kw: NC.BnCase('x', 'x', 'train', kw.get('R', 100), kw.get('C', 8), kw.get('ld', kw.get('C', 8)), kw.get('mis', False), 0, 0, ())      # noqa: E731
    assert NC.bn_path(K(R=512)) == 'mid' and NC.bn_path(K(R=513)) == 'chunk_vec' and NC.bn_path(K(R=16)) == 'mid' and NC.bn_path(K(R=15)) == 'small'
    assert NC.bn_path(K(R=100, C=6)) == 'small' and NC.bn_path(K(R=100, mis=True)) == 'small' and NC.bn_path(K(R=600, ld=9)) == 'chunk_scalar'
    part = [c for c in NC.bn_cases('partials')]
    two = [c for c in part if 'bn_partials_coarsen_kernel' in NC.bn_expected_kernels(c, 'plain')[0]]
    assert len(two) >= 3 and all(-(-c.R // c.chunk_rows) > 256 and c.cap > 257 for c in two) and any(c.cap == 257 for c in part if c not in two)
    col = lambda R, N, ld=None: NC.colsum_expected_kernels(NC.ColCase('x', R, N, ld or N), False)[0]      # noqa: E731
    assert [col(R, 4) for R in (127, 128, 4096, 4097)] == ['colsum_kernel', 'colsum_mid_kernel', 'colsum_mid_kernel', 'bn_partial4_kernel']
    assert col(200, 1) == 'colsum_kernel' and col(513, 1) == 'bn_partial_kernel' and col(200, 4, 5) == 'colsum_kernel' and col(200, 4, 8) == 'colsum_mid_kernel'
    seen = collections.Counter()
    for c in NC.bn_cases():
        fwd, bwd = NC.bn_expected_kernels(c, 'plain')
        seen.update(set(fwd) | set(bwd))
    for c in NC.colsum_cases():
        seen.update(set(NC.colsum_expected_kernels(c, False)) | set(NC.colsum_expected_kernels(c, True)))
    named = ('bn_train_fwd_kernel', 'bn_train_bwd_kernel', 'bn_mid_fwd_kernel', 'bn_mid_bwd_kernel', 'bn_stats4_kernel', 'bn_stats_combine_kernel',
             'bn_apply_fwd4_kernel', 'bn_partial_kernel', 'bn_partial4_kernel', 'bn_partials_coarsen_kernel', 'bn_stats_local_kernel',
             'bn_stats_combine_pre_kernel', 'bn_sync_combine_kernel', 'bn_bwd_sums_kernel', 'bn_bwd_partial4_kernel', 'bn_bwd_combine_kernel',
             'bn_apply_bwd4_kernel', 'bn_apply_bwd_kernel', 'bn_apply_fwd_kernel', 'bn_colsum_chunks_kernel', 'bn_stats_finalize_kernel',
             'bn_frozen_stats_kernel', 'zero_f32_kernel', 'colsum_kernel', 'colsum_mid_kernel', 'wgrad_reduce_kernel')
    assert all(seen[k] >= 3 for k in named), {k: seen[k] for k in named if seen[k] < 3}
    for cls in NC.BN_CLASSES:                                         # and, class by class, the kernels the class is there to reach
        for v in NC.BN_VARIANTS:
            for k in NC.bn_class_kernels(cls, v):
                n = sum(k in fb[0] + (fb[1] if v != 'relu_res' else []) for fb in (NC.bn_expected_kernels(c, v) for c in NC.bn_cases(cls)))
                assert n >= 3, (cls, v, k, n)


# ------------------------------------------------------------------------------------------------------------------------------ the operands
def test_operands_have_the_stated_structure():
    case = [c for c in NC.bn_cases('chunk_vec') if (c.R, c.C) == (4101, 68)][0]
    o = bn_operands(case, 'plain')
    assert all(np.array_equal(o[k], NC.bn_make(case, 'plain')[k]) for k in ('x', 'w', 'b', 'gy'))          # deterministic
    x = o['x'].astype(np.float64)
    for c in range(case.C):
        mu, sg = NC.PAIRS[c % 8]
        xc = x[:, c] - (100.0 * (np.arange(case.R) < (case.R + 1) // 2) if c == 8 else 0.0)
        assert abs(xc.mean() - mu) <= 0.1 * sg + 1e-6 * abs(mu) and abs(xc.std() - sg) <= 0.1 * sg + 1e-7 * abs(mu), c
    assert x[:2051, 8].mean() - x[2051:, 8].mean() > 99                                     # chunk means differ by 100 sigma
    assert np.all(x[:, 5] == 7.0)                                                           # a constant channel
    e = np.log2(np.abs(o['gy']).astype(np.float64).mean(0) / np.sqrt(2 / np.pi))
    assert np.abs(e - ((5 * np.arange(case.C)) % 17 - 8)).max() < 0.2 and e.min() < -7.5 and e.max() > 7.5
    r = bn_operands(case, 'relu')
    xr = r['x'].astype(np.float64)
    assert (np.abs(xr).max(0) / np.sqrt(xr.var(0) + NC.EPS)).max() <= NC.KAPPA_RELU and np.array_equal(r['x'][:, 0], o['x'][:, 0])
    s = [c for c in NC.bn_cases('sync') if len(c.splits) == 3 and c.C == 20][0]
    xs = NC.bn_make(s, 'plain')['x'].astype(np.float64)
    assert abs(xs[:300, 4].mean() - xs[301:, 4].mean()) > 100 * 30 * 1.9                    # ranks 0 and 2 of the (-50, 30) channel: 200 sigma apart
    fz = NC.bn_make(NC.bn_cases('frozen')[0], 'plain')
    assert {0.0, np.float32(1e-12), np.float32(1e6)} <= set(fz['rv0'].tolist())
    ln = NC.ln_make([c for c in NC.ln_cases() if (c.R, c.C) == (113, 128)][0])
    assert np.all(ln['x'][5] == 7.0) and ln['x'][4].max() == 1e4 and abs(ln['x'][6].mean() - 3e4) < 1
    big = NC.att_make([c for c in NC.att_cases() if c.kind == 'large' and c.T == 64][0])
    q, k, _ = NC._qkv64(big)
    assert 200 < np.abs(q @ k.transpose(0, 1, 3, 2) * big['scale']).max() < 1000
    one = [c for c in NC.att_cases() if c.kind == 'onehot' and c.T == 42][0]
    assert (NC.att_fwd_ref(NC.att_make(one), one)['probs'][0].max(-1) > 1 - 1e-6).all()
    uni = [c for c in NC.att_cases() if c.kind == 'uniform' and c.T == 21][0]
    assert np.abs(NC.att_fwd_ref(NC.att_make(uni), uni)['probs'][0] - 1 / 21).max() < 1e-12
    g = NC.gelu_make(NC.gelu_cases()[4])['x']
    assert np.isfinite(g).all() and set(np.abs(g).tolist()) == set(np.array(NC.GELU_VALUES, np.float32).tolist())


# ------------------------------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize('cls', ('small', 'mid', 'chunk_vec', 'chunk_scalar', 'strided'))
def test_batchnorm_reference_agrees_with_torch_float64_autograd(cls):
    worst = 0.0
    for case in NC.bn_cases(cls):
        if case.R == 1:
            continue                                                  # torch refuses one value per channel
        for v in ('plain', 'relu'):
            o = bn_operands(case, v)
            x = torch.from_numpy(o['x']).double().requires_grad_(True)
            w, b = (torch.from_numpy(o[k]).double().requires_grad_(True) for k in ('w', 'b'))
            rm, rv = torch.from_numpy(o['rm0']).double(), torch.from_numpy(o['rv0']).double()
            y = torch.nn.functional.batch_norm(x, rm, rv, w, b, True, NC.MOMENTUM, NC.EPS)
            y = torch.relu(y) if o['relu'] else y
            y.backward(torch.from_numpy(o['gy']).double())
            x64 = o['x'].astype(np.float64)
            st = NC.bn_stats_ref(x64, NC.bn_levels(case))
            pre, S = NC.bn_y_ref(x64, o['w'], o['b'], st['mean'], st['rstd'], st['S_mean'])
            mask = pre > 0 if o['relu'] else None
            (rmr, Srm), (rvr, Srv) = NC.bn_running_ref(st, o['rm0'], o['rv0'])
            bw = NC.bn_bwd_ref(o['gy'], x64, o['w'], st['mean'], st['rstd'], mask)
            for got, ref, Sx in ((y, np.where(mask, pre, 0) if o['relu'] else pre, S), (rm, rmr, Srm), (rv, rvr, Srv), (x.grad, ) + bw['gx'],
                                 (w.grad, ) + bw['gw'], (b.grad, ) + bw['gb']):
                worst = max(worst, NC.ratio(got.detach().numpy(), ref, np.broadcast_to(Sx, np.shape(ref))))
    assert worst < 1e-3, worst                                        # in units of 2^-24 S: float64 against float64


def test_layernorm_attention_gelu_references_agree_with_torch_float64_autograd():
    worst = 0.0
    for case in NC.ln_cases():
        o = NC.ln_make(case)
        x, w, b = (torch.from_numpy(o[k]).double().requires_grad_(True) for k in ('x', 'w', 'b'))
        y = torch.nn.functional.layer_norm(x, (case.C,), w, b, case.eps)
        y.backward(torch.from_numpy(o['gy']).double())
        f = NC.ln_fwd_ref(o, case)
        bw = NC.ln_bwd_ref(o, f['mean'][0], f['rstd'][0])
        for got, (ref, S) in ((y, f['y']), (x.grad, bw['gx']), (w.grad, bw['gw']), (b.grad, bw['gb'])):
            if case.C > 1 or got is y:                                # (one column: torch's expanded backward is not exact even in float64)
                worst = max(worst, NC.ratio(got.detach().numpy(), ref, S))
    assert worst < 2e-2, worst                                        # (torch's expanded LayerNorm backward: ~1e6 units in float32, x 2^-29 here)
    worst = 0.0
    for case in NC.att_cases():
        o = NC.att_make(case)
        B, T, H, D = case.B, case.T, case.H, NC.ATT_D
        qkv = torch.from_numpy(o['qkv']).double().requires_grad_(True)
        q, k, v = (qkv.permute(2, 0, 3, 1, 4)[j] for j in range(3))
        p = torch.softmax(q @ k.transpose(-1, -2) * o['scale'], -1)
        out = (p @ v).transpose(1, 2).reshape(B * T, H * D)
        out.backward(torch.from_numpy(o['gout']).double().reshape(B * T, H * D))
        f = NC.att_fwd_ref(o, case)
        g, Sg = NC.att_bwd_ref(o, case, f['probs'][0])
        for got, ref, S in ((p, ) + f['probs'], (out, ) + f['out'], (qkv.grad.reshape(B * T, -1), g, Sg)):
            worst = max(worst, NC.ratio(got.detach().numpy(), ref, S))
    for case in NC.gelu_cases():
        o = NC.gelu_make(case)
        x = torch.from_numpy(o['x']).double().requires_grad_(True)
        y = torch.nn.functional.gelu(x)
        y.backward(torch.from_numpy(o['gy']).double())
        r = NC.gelu_ref(o)
        worst = max(worst, NC.ratio(y.detach().numpy(), *r['y']), NC.ratio(x.grad.numpy(), *r['gx']))
    assert worst < 1e-3, worst


def test_partials_and_sync_references_are_the_whole_batch_statistics():
    """the statistics from stored chunk partials, and SyncBN's, are the plain statistics of the same rows"""
    for case in NC.bn_cases('partials')[::4] + NC.bn_cases('sync')[::3]:
        o = bn_operands(case, 'plain')
        x64 = o['x'].astype(np.float64)
        st = NC.bn_stats_ref(x64, NC.bn_levels(case), (o['p1'], o['p2']) if case.api == 'partials' else None)
        assert NC.ratio(st['mean'], x64.mean(0), st['S_mean']) < 2 * 64 and NC.ratio(st['var'], x64.var(0), st['S_var']) < 2 * 64     # float32 partials: <= rows per chunk
        assert np.all(st['S_var'] >= st['var'])


# ------------------------------------------------------------------------------------------------------------------------------ the references' error
def test_both_float32_references_stay_inside_the_bound_at_a_quarter_of_c():
    tot = survey()
    print('\n%-11s %12s %12s   c' % ('kind', 'numpy', 'torch'))
    for k in NC.RATIOS:
        a, b = tot['np_capped'].ratios.get(k, (0.0, ''))[0], tot['torch'].ratios.get(k, (0.0, ''))[0]
        print('%-11s %12.4g %12.4g   %.4g   %s' % (k, a, b, NC.C[k], tot['np_capped'].ratios.get(k, (0, ''))[1]))
        assert max(a, b) <= NC.RATIOS[k] == NC.C[k] / 4, (k, a, b)              # both pass check at c / 4 ...
        assert max(a, b) >= 0.5 * NC.RATIOS[k], (k, a, b)                       # ... and c is not padded
    assert not tot['np_capped'].failures, tot['np_capped'].failures[:5]        # the kernel-order evaluation also inside the serial caps
    assert 0 < tot['np_capped'].band <= NC.BAND_CAP and tot['torch'].band <= NC.BAND_CAP          # the undecided band of every ReLU case
    assert NC.C_MEAN >= tot['np_capped'].ratios['bn_mean'][0]


# ------------------------------------------------------------------------------------------------------------------------------ single defects
BN_DEFECT_VARIANTS = {'one_pass': ('plain',), 'drop_nkd2': ('plain',), 'last_full': ('plain',), 'biased_running': ('plain',), 'row_tail': ('plain', 'relu'),
                      'quad_tail': ('plain',), 'mask_no_bias': ('relu', 'relu_res'), 'padded_rows': ('plain', 'relu'), 'sync_no_rank_mean': ('plain',)}


@pytest.mark.parametrize('defect', NC.BN_DEFECTS)
def test_check_rejects_single_batchnorm_defects(defect):
    n = 0
    for case in NC.bn_cases():
        for v in BN_DEFECT_VARIANTS[defect]:
            if not NC.bn_defect_applies(defect, case, v):
                continue
            o = bn_operands(case, v)
            bad = NC.bn_standin32(case, v, o, defect)
            if defect == 'mask_no_bias' and np.array_equal(bad['y'], NC.bn_standin32(case, v, o)['y']):
                continue                                              # (no element of this case has the bias decide its sign)
            assert NC.bn_judge(case, v, o, bad).failures, (defect, case.name, v)
            n += 1
    assert n >= 8, n


def test_check_rejects_single_layernorm_attention_gelu_defects():
    n = collections.Counter()
    for case in NC.ln_cases():
        if case.C % 64:
            o = NC.ln_make(case)
            assert NC.ln_judge(case, o, NC.ln_standin(case, o, 'plain', pad_mean=True), 'plain').failures, case.name
            n['pad_mean'] += 1
    for case in NC.att_cases():
        o = NC.att_make(case)
        for d in ('no_max', 'drop_last', 'gk_no_scale'):
            if NC.att_defect_applies(d, case):
                assert NC.att_judge(case, o, NC.att_standin(case, o, defect=d)).failures, (d, case.name)
                n[d] += 1
    for case in NC.gelu_cases():
        o = NC.gelu_make(case)
        if np.any((np.abs(o['x']) >= 0.5) & (np.abs(o['x']) <= 4)):
            assert NC.gelu_judge(case, o, NC.gelu32(o, tanh=True)).failures, case.name
            n['tanh'] += 1
    assert all(n[d] >= 6 for d in ('pad_mean', 'no_max', 'drop_last', 'gk_no_scale', 'tanh')), n


# ------------------------------------------------------------------------------------------------------------------------------ the old gates
def rel(a, b):
    """tests/test_gpu_train_ops.py's gate: the largest difference over the largest reference value"""
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64).reshape(b.shape) - b).max() / (np.abs(b).max() + 1e-30))


def test_which_defects_the_max_norm_gates_let_through_on_their_own_data():
    """test_batchnorm_relu_fused's data (sigma in [0.5, 3], mean ~ N(0, 2)) and gates (5e-6 y and running statistics, 3e-5 gx, 1e-5 gw / gb), the
    float32 stand-in with one defect in the kernel's place, on the shapes at which the old tests reach the defect's code path: which defects pass
    every gate.  And the old gates cannot be pointed at the sweep's data: a correct float32 evaluation is 1e-4 from float64 there in max-norm."""
    hostile = [c for c in NC.bn_cases('chunk_vec') if (c.R, c.C) == (4101, 68)][0]
    ho = bn_operands(hostile, 'plain')
    st = NC.bn_stats_ref(ho['x'].astype(np.float64), NC.bn_levels(hostile))
    pre, _ = NC.bn_y_ref(ho['x'].astype(np.float64), ho['w'], ho['b'], st['mean'], st['rstd'], st['S_mean'])
    assert rel(NC.bn_standin32(hostile, 'plain', ho)['y'], pre) > 5e-6
    visits = {'quad_tail': lambda c: NC.bn_path(c) == 'mid' and c.C % 16 != 0, 'row_tail': lambda c: c.R % 4 != 0 and NC.bn_path(c) == 'chunk_vec',
              'last_full': lambda c: c.R > 512 and c.R % 256 != 0, 'padded_rows': lambda c: c.R > 512 and c.R % 256 != 0,
              'drop_nkd2': lambda c: c.R > 512}
    passed = {}
    for defect in ('one_pass', 'drop_nkd2', 'last_full', 'biased_running', 'row_tail', 'quad_tail', 'mask_no_bias', 'padded_rows'):
        ok = True
        for R, Cn, relu in ((300, 128, False), (5000, 64, True), (4097, 6, False), (1537, 36, True)):
            rng = np.random.RandomState(R + Cn)
            case = NC.BnCase('old', 'old', 'train', R, Cn, Cn, False, 0, 0, ())
            v = 'relu' if relu else 'plain'
            if not visits.get(defect, lambda c: True)(case):
                continue
            o = NC.bn_make(case, v)
            o['x'] = (rng.normal(0, 1, (R, Cn)) * rng.uniform(0.5, 3, Cn) + rng.normal(0, 2, Cn)).astype(np.float32)
            o['gy'] = rng.normal(0, 1, (R, Cn)).astype(np.float32)
            o['rm0'], o['rv0'] = np.zeros(Cn, np.float32), np.ones(Cn, np.float32)
            got = NC.bn_standin32(case, v, o, defect)
            x64 = o['x'].astype(np.float64)
            st = NC.bn_stats_ref(x64, NC.bn_levels(case))
            pre, _ = NC.bn_y_ref(x64, o['w'], o['b'], st['mean'], st['rstd'], st['S_mean'])
            mask = got['y'] > 0 if relu else None                     # (the old test takes the kernel's mask)
            (rm, _), (rv, _) = NC.bn_running_ref(st, o['rm0'], o['rv0'])
            bw = NC.bn_bwd_ref(o['gy'], x64, o['w'], st['mean'], st['rstd'], mask)
            ok = ok and (rel(got['y'], np.maximum(pre, 0) if relu else pre) < 5e-6 and rel(got['running_mean'], rm) < 5e-6 and rel(got['running_var'], rv) < 5e-6
                         and rel(got['gx'], bw['gx'][0]) < 3e-5 and rel(got['gw'], bw['gw'][0]) < 1e-5 and rel(got['gb'], bw['gb'][0]) < 1e-5
                         and (not relu or float(np.mean(mask != (pre > 0))) < 1e-5))
        passed[defect] = ok
    # LayerNorm at C = 64, 128, 256 only, attention on N(0, 1) logits, no SyncBN shape with unequal ranks: these defects change nothing the old tests run
    for case, d in ((NC.LnCase('old', 126, 128, 1e-6), 'pad_mean'),):
        o = NC.ln_make(case)
        passed[d] = all(np.array_equal(NC.ln_standin(case, o, 'plain', pad_mean=True)[k], NC.ln_standin(case, o, 'plain')[k]) for k in ('y', 'mean', 'rstd'))
    case = NC.AttCase('old', 'normal', 3, 42, 4)
    o = NC.att_make(case)
    f = NC.att_fwd_ref(o, case)
    got = NC.att_standin(case, o, defect='no_max')
    passed['no_max'] = rel(got['out'], f['out'][0]) < 3e-6 and rel(got['probs'], f['probs'][0]) < 3e-6
    print('\nlet through by the max-norm gates:', sorted(k for k, v in passed.items() if v), '| caught:', sorted(k for k, v in passed.items() if not v))
    assert passed['quad_tail'] and passed['pad_mean'] and passed['no_max']          # code paths and data the old tests never visit
