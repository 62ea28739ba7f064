"""CPU-only: the validation metric of the training loop against the reference's own function (G24, tools/gen_val_metric_golden.py:
InterHandDataset.evaluate on float32 inputs and on float64 copies of them), dir_amd.optim.MultiStepLR against torch's, and the host-side
contracts of the training driver (no CPU fallback, argument checks before any launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import val_metric_ref as R  # noqa: E402

TOL_FACTOR = 8          # the kernel's allowance in units of the reference's own float32 error d (fused multiply-adds, another summation order)


@pytest.fixture(scope='module')
def cases():
    g = dict(np.load(os.path.join(HERE, 'golden', 'g24_val_metrics.npz')))
    return g, R.fixture_cases(g)


def test_fixture_covers_the_cases_and_regenerates(cases):
    g, cs = cases
    assert {1, 5, 64} <= {c['B'] for c in cs} and {3, 5} <= {c['n_stages'] for c in cs} and any(c['exact'] for c in cs)
    for c in cs:
        outs_list, targets = R.make_case(c['seed'], c['B'], c['n_stages'], c['exact'])
        assert R.checksum(outs_list, targets) == c['checksum']
        assert c['ref32'].dtype == np.float32 and c['ref64'].dtype == np.float64 and c['ref32'].shape == c['ref64'].shape == (c['n_stages'], 4)
    outs_list, targets = R.make_case(cs[0]['seed'], cs[0]['B'], cs[0]['n_stages'])           # case 0's tensors are stored as well
    for k, v in targets.items():
        np.testing.assert_array_equal(g['in.0.gt.' + k], v)
    for s, o in enumerate(outs_list):
        for k, v in o.items():
            np.testing.assert_array_equal(g['in.0.s%d.%s' % (s, k)], v)
    d = R.fixture_d(cs)
    assert 1e-7 < d < 1e-4, d                        # float32 on errors of 10-20 mm: a few 1e-6 mm


def test_numpy_restatement_reproduces_the_reference(cases):
    _, cs = cases
    d = R.fixture_d(cs)
    for c in cs:
        outs_list, targets = R.make_case(c['seed'], c['B'], c['n_stages'], c['exact'])
        for s, o in enumerate(outs_list):
            r64 = R.evaluate_np(o, targets, np.float64)
            r32 = R.evaluate_np(o, targets, np.float32)
            assert r32.dtype == np.float32
            if c['exact']:
                assert not r64.any() and not r32.any() and not c['ref64'][s].any() and not c['ref32'][s].any()
                continue
            assert np.max(np.abs(r64 - c['ref64'][s]) / np.abs(c['ref64'][s])) < 1e-12
            assert np.max(np.abs(r32.astype(np.float64) - c['ref64'][s])) <= TOL_FACTOR * d
            assert c['ref32'][s].min() > 5              # errors of several mm: root and scale alignment did their work


def test_restatement_degenerate_bone_is_not_special_cased():
    outs_list, targets = R.make_case(7, 2, 1)
    o = outs_list[0]
    o['pd_joint_xyz_left'][1, 9] = o['pd_joint_xyz_left'][1, 0]          # a predicted bone of length 0: scale = inf
    r = R.evaluate_np(o, targets, np.float32)
    assert not np.isfinite(r[0]) and not np.isfinite(r[2]) and np.isfinite(r[1]) and np.isfinite(r[3])


def test_multistep_lr_equals_torch():
    from dir_amd.optim import MultiStepLR

    class Opt(object):
        def __init__(self):
            self.param_groups = [{'lr': 5e-4, 'initial_lr': 5e-4}]
    for milestones, gamma in (([30], 0.1), ([10, 20, 20, 45], 0.3)):
        p = torch.nn.Parameter(torch.zeros(1))
        to = torch.optim.AdamW([{'params': [p], 'initial_lr': 5e-4}], 5e-4)
        ts = torch.optim.lr_scheduler.MultiStepLR(to, milestones, gamma=gamma, last_epoch=-1)
        mo = Opt()
        ms = MultiStepLR(mo, milestones, gamma=gamma, last_epoch=-1)
        for epoch in range(50):
            assert mo.param_groups[0]['lr'] == to.param_groups[0]['lr'], epoch
            assert ms.get_last_lr() == ts.get_last_lr()
            sd, tsd = ms.state_dict(), ts.state_dict()
            assert set(sd) <= set(tsd) and all(sd[k] == tsd[k] for k in sd), (sd, tsd)
            if epoch == 33:                              # round trip, both directions
                mo2, to2 = Opt(), torch.optim.AdamW([{'params': [p], 'initial_lr': 5e-4}], 5e-4)
                ms2, ts2 = MultiStepLR(mo2, [1]), torch.optim.lr_scheduler.MultiStepLR(to2, [1])
                ms2.load_state_dict(tsd)
                ts2.load_state_dict(sd)
                assert ms2.state_dict() == sd and mo2.param_groups[0]['lr'] == mo.param_groups[0]['lr']
                assert ts2.last_epoch == ts.last_epoch and ts2.milestones == ts.milestones and ts2.get_last_lr() == ts.get_last_lr()
                mo, ms = mo2, ms2
            to.step()
            ts.step()
            ms.step()
        assert mo.param_groups[0]['lr'] < 5e-4


def test_driver_has_no_cpu_fallback(tmp_path):
    from dir_amd import _capi
    from dir_amd.apps import train as T
    outs_list, targets = R.make_case(3, 2, 3)
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(_capi.DirHipError):
        T.ValMetrics(3).update([t(o) for o in outs_list], t(targets))
    with pytest.raises(ValueError):
        T.ValMetrics(9)
    assert T.ValMetrics(3).result()['batches'] == 0

    class Tiny(torch.nn.Module):                         # any module whose parameters live on the CPU
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(_capi.DirHipError):
        T.validate(Tiny(), [])
    with pytest.raises(_capi.DirHipError):
        T.fit(Tiny(), [], output_root=str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()               # refused before anything was written


def test_driver_helpers_on_the_host():
    from dir_amd.apps import train as T
    T.check_finite(3.5, 0, 0)
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(T.NonFiniteLoss):
            T.check_finite(bad, 1, 100)
    line = T.log_line(1, 50, 100, 2000, 5e-4, {'seg': 0.12345, 'joint_uv_0': 1.0})
    assert line == '[Epoch 1/50][Batch 100/2000][lr 0.000500][loss_seg: 0.1235][loss_joint_uv_0: 1.0000]'       # train.py:72-75
    a, b = T.epoch_rng(3, 1).permutation(16), T.epoch_rng(3, 1).permutation(16)
    assert np.array_equal(a, b) and not np.array_equal(a, T.epoch_rng(3, 2).permutation(16)) and not np.array_equal(a, T.epoch_rng(4, 1).permutation(16))
    res = {'MPJPE_%d' % s: {'left': 1.0, 'right': 3.0, 'all': 2.0} for s in range(3)}
    res.update({'MPVPE_%d' % s: {'left': 2.0, 'right': 4.0, 'all': 3.0} for s in range(3)})
    printed, logged = T.report_lines(res, 3)
    assert printed[:3] == ['MPJPE_0:', '    left: 1.0 mm, right: 3.0 mm', '    all: 2.0 mm'] and len(printed) == 18       # train.py:183-188
    assert logged[1] == 'MPVPE_0: left 2.0 mm, right 4.0 mm, AVG 3.0 mm' and len(logged) == 6                            # train.py:190-199
    opt = T.build_parser().parse_args(['--init', 'x.pth'])
    assert (opt.total_epoch, opt.bs, opt.lr, opt.lr_scheduler, opt.workers, opt.seed, opt.eval_split, opt.eval_interval, opt.print_iter,
            opt.draw_iter, opt.step, opt.init_scope, opt.eval_dtype) == (50, 64, 5e-4, 'cosine', 8, 0, 'test', 1, 100, 100, 'graphed', 'all', 'f16')
    with pytest.raises(SystemExit):
        T.build_parser().parse_args([])                  # --init is required


def test_val_metrics_entry_point_host_side_contract():
    """argument checks fail with an error code and a message before anything touches a device"""
    from dir_amd import _capi
    L = _capi.lib()
    one = 16

    def desc(n_stages=3, **holes):
        d = _capi.ValMetricsDesc()
        for s in range(n_stages):
            for h in range(2):
                d.joints_pd[s][h], d.verts_pd[s][h] = one, one
        for h in range(2):
            d.joints_gt[h], d.verts_gt[h] = one, one
        d.sample_sums, d.acc, d.batches = one, one, one
        for k, v in holes.items():
            setattr(d, k, v)
        return d

    def bad(rc, word):
        assert rc != 0 and word in L.dir_last_error(), (rc, L.dir_last_error())
    bad(L.dir_val_metrics_forward(None, 3, 4, None), b'null descriptor')
    bad(L.dir_val_metrics_forward(desc(), 3, -1, None), b'B=-1')
    bad(L.dir_val_metrics_forward(desc(), 0, 4, None), b'n_stages=0')
    bad(L.dir_val_metrics_forward(desc(8), 9, 4, None), b'n_stages=9')
    bad(L.dir_val_metrics_forward(desc(2), 3, 4, None), b'null pointer (stage 2')
    bad(L.dir_val_metrics_forward(desc(acc=None), 3, 4, None), b'null pointer (sample_sums')
    bad(L.dir_val_metrics_forward(desc(batches=None), 3, 4, None), b'null pointer')
    d = desc()
    d.verts_gt[1] = None
    bad(L.dir_val_metrics_forward(d, 3, 4, None), b'ground truth, hand 1')
    assert L.dir_val_metrics_forward(desc(), 3, 0, None) == 0          # empty batch: nothing to do
    assert ctypes.sizeof(_capi.ValMetricsDesc) == 8 * (2 * 8 * 2 + 2 + 2 + 3)
