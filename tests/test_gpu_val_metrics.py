"""GPU: dir_val_metrics_forward (dir_amd.apps.train.ValMetrics) against the reference's own InterHandDataset.evaluate (G24).

Tolerance, from the reference itself: d = the largest |ref32 - ref64| over the fixture's cases (the reference's float32 result against
the same function on float64 copies of the inputs).  The kernel does the per-point maths in fp32 in the reference's order and sums in
fp64, so its distance from ref64 is of the same kind; it gets 8 d (fused multiply-adds, another summation order).  Predictions equal to
the ground truth give exactly 0."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import val_metric_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_FACTOR = 8


@pytest.fixture(scope='module')
def cases():
    return R.fixture_cases(dict(np.load(os.path.join(HERE, 'golden', 'g24_val_metrics.npz'))))


def dev(d):
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def table(res, n_stages):
    """ValMetrics.result() -> [n_stages,4] (joint L, joint R, vert L, vert R)"""
    return np.array([[res['MPJPE_%d' % s]['left'], res['MPJPE_%d' % s]['right'], res['MPVPE_%d' % s]['left'], res['MPVPE_%d' % s]['right']]
                     for s in range(n_stages)])


def run(case, metrics=None):
    from dir_amd.apps.train import ValMetrics
    outs_list, targets = R.make_case(case['seed'], case['B'], case['n_stages'], case['exact'])
    m = ValMetrics(case['n_stages']) if metrics is None else metrics
    m.update([dev(o) for o in outs_list], dev(targets))
    return m


def test_kernel_matches_the_reference_within_its_own_float32_error(cases):
    d = R.fixture_d(cases)
    worst = 0.0
    for c in cases:
        res = run(c).result()
        got = table(res, c['n_stages'])
        assert res['batches'] == 1
        if c['exact']:
            assert not got.any(), got                                   # exactly 0
            continue
        e = float(np.max(np.abs(got - c['ref64'])))
        worst = max(worst, e)
        print('B %2d stages %d: |kernel - ref64| %.3g mm, |ref32 - ref64| %.3g mm' % (
            c['B'], c['n_stages'], e, np.max(np.abs(c['ref32'].astype(np.float64) - c['ref64']))))
        last = c['n_stages'] - 1
        assert res['error'] == (got[last, 0] + got[last, 1]) / 2 and res['MPVPE_0']['all'] == (got[0, 2] + got[0, 3]) / 2
    print('d = %.3g mm, worst |kernel - ref64| = %.3g mm, allowed %.3g mm' % (d, worst, TOL_FACTOR * d))
    assert worst <= TOL_FACTOR * d, (worst, d)


def test_accumulation_over_three_batches_is_the_mean_of_the_batch_values(cases):
    three = [c for c in cases if c['B'] == 5 and c['n_stages'] == 3 and not c['exact']][:3]
    assert len(three) == 3
    from dir_amd.apps.train import ValMetrics
    m = ValMetrics(3)
    for c in three:
        run(c, m)
    res = m.result()
    want = sum(c['ref64'] for c in three) / 3
    assert res['batches'] == 3
    assert np.max(np.abs(table(res, 3) - want)) <= TOL_FACTOR * R.fixture_d(cases)
    m.reset()
    run(three[0], m)
    assert m.result()['batches'] == 1 and np.array_equal(table(m.result(), 3), table(run(three[0]).result(), 3))


def test_two_calls_give_identical_bits_and_stages_are_independent(cases):
    from dir_amd.apps.train import ValMetrics
    c = next(c for c in cases if c['B'] == 64 and c['n_stages'] == 5 and not c['exact'])
    a, b = run(c), run(c)
    assert torch.equal(a.acc, b.acc) and torch.equal(a.sample_sums, b.sample_sums) and int(a.batches[0]) == 1
    outs_list, targets = R.make_case(c['seed'], c['B'], c['n_stages'])
    t = dev(targets)
    for s in range(5):                                                   # one call with 5 stages = five single-stage calls
        m = ValMetrics(1)
        m.update([dev(outs_list[s])], t)
        assert torch.equal(m.acc[0], a.acc[s]) and torch.equal(m.sample_sums[0], a.sample_sums[s])
    # the per-sample sums are what the means are made of
    want = a.sample_sums.sum(1).cpu().numpy() / (64 * np.array([21, 21, 778, 778])) * 1000
    assert np.max(np.abs(a.acc.cpu().numpy() - want)) < 1e-9


def test_degenerate_bone_gives_non_finite_like_the_reference():
    from dir_amd.apps.train import ValMetrics
    outs_list, targets = R.make_case(7, 2, 1)
    o = outs_list[0]
    o['pd_joint_xyz_left'][1, 9] = o['pd_joint_xyz_left'][1, 0]
    ref = R.evaluate_np(o, targets, np.float32)
    m = ValMetrics(1)
    m.update([dev(o)], dev(targets))
    got = table(m.result(), 1)[0]
    assert list(np.isfinite(got)) == list(np.isfinite(ref)) == [False, True, False, True]
    assert abs(got[1] - ref[1]) < 1e-4 and abs(got[3] - ref[3]) < 1e-4


def test_update_checks_shapes():
    from dir_amd import _capi
    from dir_amd.apps.train import ValMetrics
    outs_list, targets = R.make_case(7, 2, 3)
    outs = [dev(o) for o in outs_list]
    outs[1]['pd_mesh_xyz_right'] = outs[1]['pd_mesh_xyz_right'][:, :700]
    with pytest.raises(_capi.DirHipError):
        ValMetrics(3).update(outs, dev(targets))
    with pytest.raises(ValueError):
        ValMetrics(3).update(outs[:2], dev(targets))
