"""CPU-only: the restatement of dir_mano_fit's rule (tests/helpers/mano_fit_ref.py) is what it says it is, and the constants the GPU test
(tests/test_gpu_mano_fit.py) gates with are re-measured here -- on the restatement, never on the kernel.

Measured here (float64 unless stated; the canonical hands of mano_fit_ref.truth, both sides):
  cold start from neutral_para, vertex term only (w_verts 1e4), lr 0.1: worst sample's vertex RMS 43 mm -> 0.70 mm after 100 iterations,
      0.003 mm after 200; at lr 0.03, 400 iterations: asserted below 0.1 mm
  refinement from truth + noise (0.05 root, 0.15 PCA, 0.03 cam), 2-D term only, w_init 1e-3, betas frozen, lr 0.01, 100 iterations: worst
      2-D RMS 0.071 -> 0.0092 (right), 0.086 -> 0.0088 (left) crop units = 7.7 x and 9.8 x; betas unmoved, exactly
  lr 1e3 alone does NOT overflow (Adam's steps are lr-sized whatever the gradient: |p| stays below 1.4e4 over 50 steps); with w_verts 1e20 the
      second step's v overflows: status bit 2 after one step taken
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import mano_cases as M  # noqa: E402
import mano_fit_ref as R  # noqa: E402

F64 = torch.float64


def test_adam_equals_torch_optim_adam_in_float64():
    """the hand-written step against torch.optim.Adam on the same gradient sequence, 20 steps, to 1e-12"""
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(3, 64, dtype=F64, generator=g)
    grads = [torch.randn(3, 64, dtype=F64, generator=g) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g)) for _ in range(20)]
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=0.07, betas=(0.9, 0.999), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pb1, pb2 = torch.ones(3, 1, dtype=F64), torch.ones(3, 1, dtype=F64)
    for gr in grads:
        q.grad = gr.clone()
        opt.step()
        p, m, v, pb1, pb2 = R.adam_step(p, gr, m, v, pb1, pb2, (0.07,) * 4, 0.9, 0.999, 1e-8)
        assert float((p - q.detach()).abs().max()) <= 1e-12
    # a group at lr 0 keeps its bits while its moments move
    p2, m2, _, _, _ = R.adam_step(p0, grads[0], torch.zeros_like(p0), torch.zeros_like(p0), torch.ones(3, 1, dtype=F64), torch.ones(3, 1, dtype=F64),
                                  (0.1, 0.1, 0.0, 0.1), 0.9, 0.999, 1e-8)
    assert torch.equal(p2[:, 51:61], p0[:, 51:61]) and not torch.equal(p2[:, :51], p0[:, :51]) and bool((m2[:, 51:61] != 0).all())


def test_gradient_is_the_backward_reference_for_the_named_cotangents():
    """residual_gradient's g = mano_cases.backward_ref (float64 autograd through the pinned restatement) for gV, gJ, gU as the header names them"""
    for config, side in (('mesh', 'right'), ('joints', 'left'), ('uv', 'right')):
        prob = R.problem(config, 2, side)
        p = torch.from_numpy(prob.init.astype(np.float64))
        g, out, mse, cot = R.residual_gradient(prob, p, F64)
        w = prob.weights
        for b in range(2):
            # the cotangents, written out once more from the targets
            exp = {'verts': np.zeros((778, 3)), 'joints': np.zeros((21, 3)), 'joint_uv': np.zeros((21, 2)), 'mesh_uv': np.zeros((778, 2))}
            if prob.verts is not None:
                exp['verts'] = 2.0 * w['w_verts'] / 778.0 * (out['verts'][b].numpy() - prob.verts[b].astype(np.float64))
            for key, tg, cf, wk in (('joints', prob.joints, prob.joints_conf, 'w_joints'), ('joint_uv', prob.joint_uv, prob.uv_conf, 'w_uv')):
                if tg is not None:
                    for j in range(21):
                        if cf[b, j] > 0:
                            exp[key][j] = 2.0 * w[wk] / 21.0 * float(cf[b, j]) * (out[key][b, j].numpy() - tg[b, j].astype(np.float64))
            for k in ('verts', 'joints', 'joint_uv'):
                assert np.abs(cot[k][b].numpy() - exp[k]).max() <= 1e-12 * max(1.0, np.abs(exp[k]).max()), (config, k)
            case = M.Case('fit_grad_%s_%s_%d' % (config, side, b), R.KIND, side, prob.center, False, 'normal', 'normal', 'fit', prob.init[b])
            M._COT[case.name] = exp
            ref = M.backward_ref(case, M.KINDS, fold=True)
            assert np.abs(g[b].numpy() - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (config, side, b)


def test_a_target_under_confidence_zero_changes_nothing():
    """NaN, infinity and finite garbage under confidence 0 give the same bits; under confidence > 0 the row passes through with status bit 1"""
    for config, key in (('joints', 'joints'), ('uv', 'joint_uv')):
        prob = R.problem(config, 2, 'right')
        tg = getattr(prob, key)
        conf = prob.joints_conf if key == 'joints' else prob.uv_conf
        assert np.isnan(tg).any() and (conf == 0).any()
        base = R.fit(prob, 5, torch.float32)
        assert base['status'].tolist() == [0, 0] and all(bool(torch.isfinite(base[k]).all()) for k in R.OUTPUTS)
        for junk in (np.inf, 12345.0):
            t2 = tg.copy()
            t2[np.isnan(tg)] = junk
            other = R.fit(prob._replace(**{key: t2}), 5, torch.float32)
            assert all(torch.equal(base[k], other[k]) for k in R.OUTPUTS + ('status',))
        c2 = conf.copy()
        c2[0][conf[0] == 0] = 0.5                       # row 0: the NaN target comes into use
        hit = R.fit(prob._replace(**{('joints_conf' if key == 'joints' else 'uv_conf'): c2}), 5, torch.float32)
        assert hit['status'].tolist() == [2, 0]
        assert torch.equal(hit['para'][0], torch.from_numpy(prob.init[0])) and torch.equal(hit['para'][1], base['para'][1])
        assert int(hit['state'][4][0]) == 0 and int(hit['state'][4][1]) == 5 and bool(torch.isfinite(hit['verts']).all())


def test_convergence_figures():
    """the figures of this file's docstring, re-measured"""
    for side in ('right', 'left'):
        cold = R.problem('mesh', 6, side)._replace(lr=(0.1,) * 4)
        rms = {it: R.fit(cold, it, F64)['mse_after'][:, 0].sqrt() * 1e3 for it in (0, 100, 200)}
        print(side, 'cold start, lr 0.1, vertex RMS mm:', {it: [round(float(x), 4) for x in r] for it, r in rms.items()})
        assert float(rms[0].min()) > 20.0 and float(rms[100].max()) < 1.0 and float(rms[200].max()) < 0.01
        r32 = R.fit(cold, 200, torch.float32)
        assert float(r32['mse_after'][:, 0].sqrt().max()) * 1e3 < 0.01 and r32['status'].tolist() == [0] * 6
        slow = R.fit(R.problem('mesh', 6, side), 400, F64)
        assert float(slow['mse_after'][:, 0].sqrt().max()) * 1e3 < 0.1
        ref = R.problem('uv', 6, side)
        r = R.fit(ref, 100, F64)
        before, after = r['mse_before'][:, 2].sqrt(), r['mse_after'][:, 2].sqrt()
        print(side, 'refinement, 2-D RMS crop units: %.4f -> %.4f (%.2f x)' % (float(before.max()), float(after.max()), float(before.max() / after.max())))
        assert float(before.max() / after.max()) > 7.0
        assert torch.equal(r['para'][:, 51:61], torch.from_numpy(ref.init[:, 51:61]).double())          # betas frozen: unmoved, exactly
        assert float((r['para'][:, :51] - torch.from_numpy(ref.init[:, :51]).double()).abs().max()) > 1e-3


def test_state_resumes_bit_for_bit_and_hostile_rows():
    prob = R.problem('uv', 2, 'left')
    whole = R.fit(prob, 10, torch.float32)
    first = R.fit(prob, 5, torch.float32)
    second = R.fit(prob, 5, torch.float32, state=first['state'], anchor=prob.init, init=first['para'].numpy())
    assert all(torch.equal(whole[k], second[k]) for k in R.OUTPUTS) and all(torch.equal(a, b) for a, b in zip(whole['state'], second['state']))
    # NaN in init: bit 1, p0's bits back, outputs 0
    bad = prob.init.copy()
    bad[1, 7] = np.nan
    r = R.fit(prob._replace(init=bad), 5, torch.float32)
    assert r['status'].tolist() == [0, 2] and np.array_equal(r['para'][1].numpy().view(np.uint32), bad[1].view(np.uint32))
    assert float(r['verts'][1].abs().max()) == 0.0 and torch.equal(r['para'][0], R.fit(prob, 5, torch.float32)['para'][0])
    # lr 1e3: finite on its own; with w_verts 1e20 the second step is refused (bit 2) and the first step's iterate comes back finite
    hot = R.problem('mesh', 3, 'right')._replace(lr=(1e3,) * 4)
    r = R.fit(hot, 50, torch.float32)
    assert r['status'].tolist() == [0, 0, 0] and float(r['para'].abs().max()) < 1.4e4
    r = R.fit(hot._replace(weights=dict(hot.weights, w_verts=1e20)), 10, torch.float32)
    assert r['status'].tolist() == [4, 4, 4] and r['state'][4].tolist() == [1, 1, 1]
    assert all(bool(torch.isfinite(r[k]).all()) for k in R.OUTPUTS) and 900.0 < float(r['para'].abs().max()) < 1100.0


def test_float32_against_float64_runs_are_the_recorded_gates():
    """GATES holds the largest |float32 run - float64 run| per (configuration, iteration count, output); the float32 restatement itself therefore
    stays inside a quarter of the GPU gate (MARGIN x the record).  A re-measured figure above its record fails; a record more than 4 x the
    re-measured figure is stale and fails too."""
    for config in ('mesh', 'joints', 'uv'):
        got = R.measure(config)
        for it in R.ITERS:
            print(config, it, {k: '%.3g (record %.3g)' % (got[it][k], R.GATES[config][it][k]) for k in R.OUTPUTS})
            for k in R.OUTPUTS:
                rec = R.GATES[config][it][k]
                assert got[it][k] <= rec, (config, it, k, got[it][k], rec)
                assert got[it][k] <= R.gate(config, it, k) / 4.0
                assert got[it][k] >= rec / 4.0, ('stale record', config, it, k, got[it][k], rec)
    # an order-dependent sign of a near-zero gradient would show as a parameter difference of the order of lr; none of the canonical cases has one
    assert max(R.GATES[c][it]['para'] for c in R.GATES for it in R.ITERS) < 2e-6
