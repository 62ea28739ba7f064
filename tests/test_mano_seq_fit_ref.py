"""CPU-only: the restatement of dir_mano_fit_sequence's rule (tests/helpers/mano_seq_fit_ref.py) is what it says it is, and the constants the GPU
test (tests/test_gpu_mano_seq_fit.py) gates with are re-measured here -- on the restatement, never on the kernel.  float64 unless stated.

Measured here and recorded in mano_seq_fit_ref.FIGURES (the inputs were chosen so that the statements hold in float64; the figures were read off
afterwards):
  shape_case (8 frames of one true shape, joints with 3 mm of noise, w_beta 0.1, 200 iterations at lr 0.03): |shared betas - truth| against
      |mean of the per-frame fits' betas - truth|; the prior pulls every per-frame fit towards 0 once per frame, the shared shape once per sequence
  canonical case, 50 iterations: the two frames without data (every confidence 0), joint RMS distance from the truth at the start (where
      mano_fit_ref.fit leaves them: it has nothing to move them with) and after the sequence fit
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import mano_fit_ref as R  # noqa: E402
import mano_seq_fit_ref as Q  # noqa: E402

F64 = torch.float64
LIVE = [n for n in range(sum(Q.LENGTHS)) if n != Q.INERT]


def _same(a, b, keys=Q.OUTPUTS, rows=slice(None)):
    return all(torch.equal(a[k][rows], b[k][rows]) for k in keys if k != 'shape')


def _rows(prob, rows):
    return prob._replace(init=prob.init[rows], joints=prob.joints[rows], joints_conf=prob.joints_conf[rows])


def test_zero_temporal_weights_and_a_shape_per_frame_are_the_independent_fit():
    """with all temporal weights 0 and per-frame shape the restatement equals mano_fit_ref.fit on the same rows exactly: every output, the status and
    the Adam state.  (The restatement evaluates one sequence at a time -- torch rounds a row differently in batches of different sizes -- so `the same
    rows` are a sequence's.)"""
    st = Q.starts_of(Q.LENGTHS)
    for side in ('right', 'left'):
        prob, _ = Q.canonical(side)
        for iters in (0, 1, 10):
            s = Q.fit_sequence(prob, Q.LENGTHS, iters, smooth=(0.0, 0.0, 0.0), share=False)
            for i in range(len(Q.LENGTHS)):
                rows = slice(int(st[i]), int(st[i + 1]))
                f = R.fit(_rows(prob, rows), iters)
                live = torch.isfinite(f['para']).all(1)
                for k in R.OUTPUTS + ('mse_before',):
                    assert torch.equal(s[k][rows][live], f[k][live]), (side, iters, i, k)
                assert s['status'][rows].tolist() == f['status'].tolist()
                assert all(torch.equal(x[rows][live], y[live]) for x, y in zip(s['state'], f['state']))
                # an inert frame: p0's bits back (NaN included), outputs 0
                assert np.array_equal(s['para'][rows].numpy().view(np.uint64), f['para'].numpy().view(np.uint64))
                assert float(s['verts'][rows][~live].abs().sum()) == 0.0
            assert s['status'].tolist() == [0, 0, 0, 0, 0, 0, Q.S_INERT, 0, 0]


def test_hand_written_gradient_is_autograd_of_the_objective_as_one_scalar():
    """temporal terms, shared shape and priors: the gradient the restatement steps along against torch.autograd of E written as one scalar, to 1e-12
    relative, at a generic point (the iterate after 3 steps) of the canonical case and of a case with every prior and a 2-frame chain"""
    for side, share in (('right', True), ('left', False), ('left', True)):
        prob, _ = Q.canonical(side)
        prob = prob._replace(weights=dict(prob.weights, w_init=1e-2))
        at = Q.fit_sequence(prob, Q.LENGTHS, 3, share=share, smooth=(0.7, 0.3, 1.9))
        p = torch.where(torch.isfinite(at['para']), at['para'], torch.zeros((), dtype=F64))
        shape = at['shape'] + 0.01
        for smooth in ((0.7, 0.3, 1.9), (0.0, 0.5, 0.0), (2.0, 0.0, 0.0)):
            g, gs = Q.gradient(prob, Q.LENGTHS, p, shape, smooth, share, F64)
            q, sh = p.clone().requires_grad_(True), shape.clone().requires_grad_(True)
            E = Q.objective(prob, Q.LENGTHS, q, sh, smooth, share, F64)
            ref = torch.autograd.grad(E, [q, sh], allow_unused=True)
            rg = ref[0].clone()
            if share:
                rg[:, 51:61] = 0
                assert float((gs - ref[1]).abs().max()) <= 1e-12 * max(1.0, float(ref[1].abs().max())), (side, smooth)
            rg[Q.INERT] = 0
            assert float((g - rg).abs().max()) <= 1e-12 * max(1.0, float(rg.abs().max())), (side, share, smooth, float((g - rg).abs().max()))
            assert float(rg[:, :6].abs().max()) > 1e-3 and float(g[Q.INERT].abs().max()) == 0.0


def test_a_sequence_alone_equals_the_same_sequence_inside_the_ragged_batch():
    prob, _ = Q.canonical('right')
    st = Q.starts_of(Q.LENGTHS)
    for share in (True, False):
        whole = Q.fit_sequence(prob, Q.LENGTHS, 6, share=share)
        for s, n in enumerate(Q.LENGTHS):
            rows = slice(int(st[s]), int(st[s + 1]))
            sub = _rows(prob, rows)
            alone = Q.fit_sequence(sub, (n,), 6, share=share)
            live = torch.isfinite(alone['para']).all(1)
            for k in Q.OUTPUTS:
                if k != 'shape':
                    assert torch.equal(alone[k][live], whole[k][rows][live]), (share, s, k)
            assert torch.equal(alone['shape'][0], whole['shape'][s]) and alone['status'].tolist() == whole['status'][rows].tolist()


def test_the_inert_frame_splits_the_chain():
    """with a shape per frame, changing a frame on one side of the inert frame changes nothing on the other side -- and does change its own side"""
    prob, _ = Q.canonical('right')
    base = Q.fit_sequence(prob, Q.LENGTHS, 8, torch.float32, share=False)
    assert base['status'].tolist() == [0, 0, 0, 0, 0, 0, Q.S_INERT, 0, 0] and base['seq_status'].tolist() == [0, 0, 0]
    jt = prob.joints.copy()
    jt[7] += 0.01
    other = Q.fit_sequence(prob._replace(joints=jt), Q.LENGTHS, 8, torch.float32, share=False)
    assert _same(base, other, rows=slice(0, 6)) and not torch.equal(base['para'][7], other['para'][7]) and not torch.equal(base['para'][8], other['para'][8])
    # with the shared shape the two chains of the sequence talk through it
    sb, so = (Q.fit_sequence(p, Q.LENGTHS, 8, torch.float32, share=True) for p in (prob, prob._replace(joints=jt)))
    assert _same(sb, so, rows=slice(0, 4)) and not torch.equal(sb['para'][4], so['para'][4])
    # two adjacent inert frames, and a non-finite target in use: bit 3, the frame stays in the chain and moves
    init = prob.init.copy()
    init[5, 0] = np.inf
    conf = prob.joints_conf.copy()
    conf[2, 4] = 0.5                                                    # frame 2's NaN targets: one comes into use
    r = Q.fit_sequence(prob._replace(init=init, joints_conf=conf), Q.LENGTHS, 8, torch.float32)
    assert r['status'].tolist() == [0, 0, Q.S_NODATA, 0, 0, Q.S_INERT, Q.S_INERT, 0, 0]
    assert not torch.equal(r['para'][2], torch.from_numpy(init[2])) and float(r['mse_after'][2].abs().max()) == 0.0
    assert torch.equal(r['para'][2, 51:61], r['shape'][1]) and torch.equal(r['para'][4, 51:61], r['shape'][2]) and torch.equal(r['para'][8, 51:61], r['shape'][2])


def test_shared_betas_are_nearer_the_truth_than_the_mean_of_the_per_frame_fits():
    for side in ('right', 'left'):
        prob, truth = Q.shape_case(side)
        bt = torch.from_numpy(truth[0, 51:61]).double()
        assert np.array_equal(truth[:, 51:61], np.repeat(truth[:1, 51:61], truth.shape[0], 0))
        shared = Q.fit_sequence(prob, (truth.shape[0],), 200, smooth=(0.0, 0.0, 0.0), share=True)
        frames = R.fit(prob, 200)
        e_shared, e_mean = float((shared['shape'][0] - bt).norm()), float((frames['para'][:, 51:61].mean(0) - bt).norm())
        print(side, 'betas: |truth| %.3f, |shared - truth| %.4f, |mean of per-frame fits - truth| %.4f' % (float(bt.norm()), e_shared, e_mean))
        assert e_shared < e_mean and shared['status'].tolist() == [0] * truth.shape[0]
        rec = Q.FIGURES['shape'][side]
        assert abs(e_shared - rec[0]) <= 0.01 * rec[0] and abs(e_mean - rec[1]) <= 0.01 * rec[1], 'the recorded figures are stale'


def test_frames_without_data_are_filled_from_their_neighbours():
    """the all-confidence-0 frames end nearer the truth than they start, and nearer than the independent fit leaves them"""
    for side in ('right', 'left'):
        prob, truth = Q.canonical(side)
        tj = R.targets_of(truth, side)['joints']
        rms = lambda r, n: float(np.sqrt(((r['joints'][n].numpy() - tj[n]) ** 2).sum(-1).mean())) * 1e3  # noqa: E731
        start, seq, alone = Q.fit_sequence(prob, Q.LENGTHS, 0), Q.fit_sequence(prob, Q.LENGTHS, 50), R.fit(prob, 50)
        for n in Q.NO_DATA:
            print(side, 'frame %d joint RMS mm: start %.2f, independent fit %.2f, sequence fit %.2f' % (n, rms(start, n), rms(alone, n), rms(seq, n)))
            assert rms(seq, n) < rms(start, n) and rms(seq, n) < rms(alone, n)
            rec = Q.FIGURES['fill'][side][n]
            assert abs(rms(start, n) - rec[0]) <= 0.01 * rec[0] and abs(rms(seq, n) - rec[1]) <= 0.01 * rec[1], 'the recorded figures are stale'
        assert seq['status'].tolist() == [0, 0, 0, 0, 0, 0, Q.S_INERT, 0, 0]


def test_five_plus_five_iterations_with_the_state_equal_ten():
    prob, _ = Q.canonical('left')
    for share in (True, False):
        whole = Q.fit_sequence(prob, Q.LENGTHS, 10, torch.float32, share=share)
        first = Q.fit_sequence(prob, Q.LENGTHS, 5, torch.float32, share=share)
        init = first['para'].numpy().copy()
        second = Q.fit_sequence(prob, Q.LENGTHS, 5, torch.float32, share=share, state=first['state'], seq_state=first['seq_state'], anchor=prob.init, init=init)
        assert _same(whole, second, rows=LIVE) and torch.equal(whole['shape'], second['shape'])
        assert all(torch.equal(a[LIVE], b[LIVE]) for a, b in zip(whole['state'], second['state']))
        assert all(torch.equal(a, b) for a, b in zip(whole['seq_state'], second['seq_state']))
        assert whole['seq_state'][4].tolist() == ([10, 10, 10] if share else [0, 0, 0]) and whole['state'][4].tolist() == [10] * 6 + [0] + [10] * 2


def test_float32_against_float64_runs_are_the_recorded_gates():
    """GATES holds the largest |float32 run - float64 run| per (configuration, iteration count, output).  A re-measured figure above its record fails;
    a record more than 4 x the re-measured figure is stale and fails too."""
    for config in Q.CONFIGS:
        got = Q.measure(config)
        for it in Q.ITERS:
            print(config, it, {k: '%.3g (record %.3g)' % (got[it][k], Q.GATES[config][it][k]) for k in Q.OUTPUTS})
            for k in Q.OUTPUTS:
                rec = Q.GATES[config][it][k]
                assert got[it][k] <= rec, (config, it, k, got[it][k], rec)
                assert got[it][k] >= rec / 4.0, ('stale record', config, it, k, got[it][k], rec)
    # an order-dependent sign of a near-zero gradient would show as a parameter difference of the order of lr (0.03): the canonical case has none
    assert max(Q.GATES[c][it]['para'] for c in Q.GATES for it in Q.ITERS) < 1e-5
