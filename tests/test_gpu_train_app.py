"""GPU: the training driver (dir_amd.apps.train: main / fit / validate) on the fake split of tests/helpers/fake_train_split.py with
synthetic weights: the files it writes, bit-equality with a hand-written TrainBatches + train_step loop, validation after training
(stale-engine pitfall), validation against the numpy restatement of the reference's metric, resume, a falling loss, and no host
synchronisation on iterations that do not print."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import val_metric_ref as R  # noqa: E402
from fake_train_split import write_train_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402

pytestmark = pytest.mark.gpu

N_IMG, BS, SEED = 8, 4, 3
TOL_FACTOR = 8
# the falling-loss run: 8 fixed images (replicated so that one epoch has LOSS_STEPS batches of 8), augment=False.  Chosen after one look at
# the curve on the MI355X ("Training driver")
LOSS_STEPS, LOSS_LR = 40, 2e-5


def is_buf(k):
    return any(t in k for t in ('running_', 'num_batches', 'mano_layer', 'img_gird', 'seg_loss.weight'))


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def mano(state):
    return DS.gt_layers_from_checkpoint(state)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    """8 train images and the same 8 as the test split"""
    d = str(tmp_path_factory.mktemp('split'))
    write_train_split(d, N_IMG, seed=11)
    shutil.copytree(os.path.join(d, 'train'), os.path.join(d, 'test'))
    return d


@pytest.fixture(scope='module')
def init_ckpt(tmp_path_factory, state):
    p = str(tmp_path_factory.mktemp('init') / 'init.pth')
    torch.save({'net': state}, p)
    return p


def make_model(state):
    from dir_amd.models.dir import DIR
    m = DIR(21, 'unused', 0, compute_dtype=torch.float16)
    m.load_state_dict(state, strict=True)
    m.autotune = False                       # kernel choices are bit-identical; the timing runs only cost time here
    return m.cuda()


def train_batches(root, mano, seed=SEED, bs=BS, **kw):
    from dir_amd.apps.trainset import TrainBatches
    return TrainBatches(root, mano, 'train', batch_size=bs, workers=2, seed=seed, **kw)


def val_batches(root, mano, bs=BS):
    from dir_amd.apps.trainset import TrainBatches
    return TrainBatches(root, mano, 'test', batch_size=bs, workers=2, seed=SEED, augment=False, shuffle=False)


def hand_written_loop(state, root, mano, epochs, lr, total_epoch):
    """what the driver must equal bit for bit: TrainBatches re-seeded per epoch + train_step + the cosine schedule"""
    from dir_amd.apps import train as T
    from dir_amd.optim import CosineAnnealingLR, FlatAdamW
    from dir_amd.train import step as TSTEP
    params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in state.items() if not is_buf(k)}
    buffers = {k: v.clone().cuda() for k, v in state.items() if is_buf(k) and 'num_batches' not in k}
    opt = FlatAdamW([{'params': list(params.values()), 'initial_lr': lr}], lr)
    opt.set_inactive(TSTEP.inactive_parameters(params))
    sched = CosineAnnealingLR(opt, T_max=total_epoch, eta_min=0)
    faces = tuple(buffers['init_regressor.mano_layer_%s.th_faces' % s] for s in ('left', 'right'))
    tb = train_batches(root, mano)
    perms = {}
    for epoch in range(epochs):
        tb.rng = T.epoch_rng(SEED, epoch)
        for inputs, targets, meta in tb:
            TSTEP.train_step(params, buffers, inputs['img'], targets, meta, faces, opt)
        perms[epoch] = np.array(tb.last_perm)
        sched.step()
    torch.cuda.synchronize()
    return {k: p.detach().clone() for k, p in params.items()}, buffers, perms, opt


@pytest.fixture(scope='module')
def by_hand(state, root, mano):
    return hand_written_loop(state, root, mano, epochs=2, lr=1e-5, total_epoch=2)


def run_fit(state, root, mano, out, step, **kw):
    from dir_amd.apps import train as T
    model = make_model(state)
    args = dict(output_root=str(out), total_epoch=2, lr=1e-5, step=step, print_iter=0, draw_iter=0, seed=SEED)
    args.update(kw)
    res = T.fit(model, train_batches(root, mano), args.pop('val', None), **args)
    torch.cuda.synchronize()
    return model, res


@pytest.mark.parametrize('step', ['eager', 'graphed'])
def test_driver_equals_the_hand_written_loop_bit_for_bit(tmp_path, state, root, mano, by_hand, step):
    want_p, want_b, want_perms, want_opt = by_hand
    model, res = run_fit(state, root, mano, tmp_path, step)
    assert res['steps'] == 4 and res['epochs'] == 2 and res['optimizer'].step_count == want_opt.step_count == 4
    got = dict(model.named_parameters())
    assert sorted(got) == sorted(want_p)
    bad = [k for k in want_p if not torch.equal(got[k].detach(), want_p[k])]
    assert not bad, (len(bad), bad[:5])
    got_b = dict(model.named_buffers())
    bad = [k for k in want_b if not torch.equal(got_b[k], want_b[k])]
    assert not bad, (len(bad), bad[:5])
    changed = sum(int(not torch.equal(want_p[k].cpu(), state[k])) for k in want_p)
    assert changed > len(want_p) // 2                                        # the steps did train
    for e in (0, 1):
        assert np.array_equal(res['perms'][e], want_perms[e])
    assert not np.array_equal(res['perms'][0], res['perms'][1])
    assert res['optimizer'].param_groups[0]['lr'] == want_opt.param_groups[0]['lr']
    # num_batches_tracked advanced as the module's own training forward advances it
    nbt = {k: int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert nbt and all(v - int(state[k]) == (8 if ('.global_pos_emb.' in k or '.proj_feat_emb.' in k) else 4) for k, v in nbt.items())


def test_command_line_writes_checkpoints_log_and_pictures(tmp_path, state, root, init_ckpt):
    from dir_amd.apps import eval as E
    from dir_amd.apps import train as T
    from dir_amd.models.dir import DIR
    out = str(tmp_path / 'out')
    res = T.main(['--data_path', root, '--output_root', out, '--init', init_ckpt, '--total_epoch', '2', '--bs', '4', '--lr', '1e-5',
                  '--workers', '2', '--print_iter', '1', '--draw_iter', '1', '--seed', '3'])
    assert res['steps'] == 4 and res['epochs'] == 2 and res['last_val']['batches'] == 2
    ck = os.path.join(out, 'checkpoint')
    assert os.path.exists(os.path.join(ck, 'latest.pth')) and os.path.exists(os.path.join(ck, 'best.pth'))
    latest = torch.load(os.path.join(ck, 'latest.pth'), map_location='cpu', weights_only=False)
    assert sorted(latest) == ['last_epoch', 'net', 'optimizer', 'schedule'] and latest['last_epoch'] == 1
    assert sorted(latest['net']) == sorted(state) and len(latest['net']) == 963
    DIR(21, 'unused', 0).load_state_dict(latest['net'], strict=True)
    assert latest['schedule']['last_epoch'] == 2 and latest['optimizer']['param_groups'][0]['initial_lr'] == 1e-5
    assert all(int(float(s['step'])) == 4 for s in latest['optimizer']['state'].values())
    log = open(os.path.join(out, 'log', 'train_DIR.log')).read()
    lines = [l for l in log.split('\n') if '[Epoch ' in l]
    assert len(lines) == 4 and '[Epoch 0/2][Batch 0/2][lr 0.000010][loss_' in lines[0] and '[Epoch 1/2][Batch 1/2][lr 0.000005]' in lines[3]
    assert lines[0].count('[loss_') == 42
    for s in range(3):
        assert log.count('MPJPE_%d: left ' % s) == 2 and log.count('MPVPE_%d: left ' % s) == 2
    assert ' mm, AVG ' in log and 'Save checkpoint to' in log
    pngs = sorted(os.listdir(os.path.join(out, 'vis')))
    # iterations 0 and 1 of either epoch write the same names: 2 iterations x 4 images x 3 stages
    assert len(pngs) == 24 and '0_pd_0.png' in pngs and '7_pd_2.png' in pngs and len(res['vis']) == 48
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(out, 'vis', pngs[0])))
    assert im.shape == (256, 256, 3) and im.std() > 1
    # apps.eval's loop accepts the checkpoint
    m = E.main(['--model', os.path.join(ck, 'latest.pth'), '--data_path', root, '--bs', '4', '--workers', '2', '--result_dir', str(tmp_path / 'res')])
    s = m.summarize()
    assert np.isfinite(s['joint_mm']['all']) and np.isfinite(s['vert_mm']['all'])


def test_validation_sees_the_trained_weights_and_equals_a_fresh_model(tmp_path, state, root, mano):
    """FlatAdamW's and BatchNorm's kernels write through raw pointers; validate() drops the packed engine first.  Validation after k steps
    differs from validation before them and equals, bit for bit, that of a fresh DIR loaded from the saved checkpoint."""
    from dir_amd.apps import train as T
    model = make_model(state)
    vb = val_batches(root, mano)
    before = T.validate(model, vb, quiet=True)
    assert model.training and before['batches'] == 2 and np.isfinite(before['error'])
    assert T.validate(model, vb, quiet=True) == before                    # same noise, same bits
    res = T.fit(model, train_batches(root, mano), vb, output_root=str(tmp_path), total_epoch=1, lr=1e-4, step='eager', print_iter=0,
                draw_iter=0, seed=SEED)
    after = T.validate(model, vb, quiet=True)
    assert res['last_val'] == after and res['min_error'] == min(100, after['error'])
    assert after != before and after['error'] != before['error'] and after['MPVPE_0'] != before['MPVPE_0']
    fresh = make_model(state)
    ck = torch.load(os.path.join(str(tmp_path), 'checkpoint', 'latest.pth'), map_location='cpu', weights_only=False)
    fresh.load_state_dict(ck['net'], strict=True)
    assert T.validate(fresh, val_batches(root, mano), quiet=True) == after


def test_validate_equals_the_reference_restatement_on_eval_outputs(state, root, mano):
    """validate() against tests/helpers/val_metric_ref.py::evaluate_np (float64) on the outputs of DIR.eval() for the same batches.
    Tolerance: 8 d as for the kernel (test_gpu_val_metrics.py), d = the reference's own float32 error on the fixture."""
    from dir_amd.apps import train as T
    cases = R.fixture_cases(dict(np.load(os.path.join(HERE, 'golden', 'g24_val_metrics.npz'))))
    d = R.fixture_d(cases)
    model = make_model(state)
    vb = val_batches(root, mano)
    got = T.validate(model, vb, quiet=True)
    vb.rng = np.random.default_rng(vb.seed)
    model.eval()
    sums, n = np.zeros((3, 4)), 0
    with torch.no_grad():
        for inputs, targets, meta in vb:
            outs_list, _ = model(inputs, targets, meta)
            t = {k: v.cpu().numpy() for k, v in targets.items() if k.startswith(('joint_3d', 'mesh_3d'))}
            for s in range(3):
                sums[s] += R.evaluate_np({k: v.float().cpu().numpy() for k, v in outs_list[s].items() if k.startswith(('pd_joint_xyz', 'pd_mesh_xyz'))},
                                         t, np.float64)
            n += 1
    want = sums / n
    have = np.array([[got['MPJPE_%d' % s]['left'], got['MPJPE_%d' % s]['right'], got['MPVPE_%d' % s]['left'], got['MPVPE_%d' % s]['right']]
                     for s in range(3)])
    tol = TOL_FACTOR * d
    print('errors %.4g .. %.4g mm, |validate - restatement| %.3g mm, allowed %.3g mm' % (want.min(), want.max(), np.max(np.abs(have - want)), tol))
    assert n == 2 and np.max(np.abs(have - want)) <= tol
    assert got['error'] == (have[2, 0] + have[2, 1]) / 2


def test_resume_continues_the_uninterrupted_run(tmp_path, state, root, mano, by_hand):
    """a run stopped after epoch 0 and continued reaches epoch 1 with the schedule's learning rate, the optimiser's step count and the batch
    indices of the uninterrupted run (the hand-written loop of the bit-equality test)"""
    _, _, want_perms, want_opt = by_hand
    _, first = run_fit(state, root, mano, tmp_path, 'eager', max_steps=2)
    assert first['steps'] == 2 and first['epochs'] == 1 and np.array_equal(first['perms'][0], want_perms[0])
    latest = os.path.join(str(tmp_path), 'checkpoint', 'latest.pth')
    assert torch.load(latest, map_location='cpu', weights_only=False)['last_epoch'] == 0
    _, second = run_fit(state, root, mano, tmp_path, 'eager', continue_train=latest)
    assert list(second['perms']) == [1] and np.array_equal(second['perms'][1], want_perms[1])
    assert second['steps'] == 2 and second['optimizer'].step_count == 4
    assert second['lrs'][1] == first['optimizer'].param_groups[0]['lr'] == 1e-5 * (1 + np.cos(np.pi / 2)) / 2
    assert second['optimizer'].param_groups[0]['lr'] == want_opt.param_groups[0]['lr']
    assert second['schedule'].last_epoch == 2
    assert torch.load(latest, map_location='cpu', weights_only=False)['last_epoch'] == 1


def test_module_step_runs_the_reference_lines(tmp_path, state, root, mano):
    """--step module: optimizer.zero_grad(); outs_list, loss = model(...); sum(loss).backward(); optimizer.step() on the module in training mode"""
    model, res = run_fit(state, root, mano, tmp_path, 'module', total_epoch=1, print_iter=1)
    totals = [t for _, t in res['printed']]
    assert res['steps'] == 2 and len(totals) == 2 and all(np.isfinite(totals))
    changed = sum(int(not torch.equal(p.detach().cpu(), state[k])) for k, p in model.named_parameters())
    assert changed > len(list(model.parameters())) // 2
    nbt = {k: int(v) - int(state[k]) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert set(nbt.values()) == {2, 4}                                     # advanced by the module's own forward, once


def replicate(root, dst, copies):
    """the 8 images of `root`/train, `copies` times over: one epoch = `copies` batches of 8 drawn from the same 8 images"""
    for kind, ext in (('img', 'jpg'), ('mask', 'jpg'), ('dense', 'jpg'), ('anno', 'pkl')):
        os.makedirs(os.path.join(dst, 'train', kind), exist_ok=True)
        for c in range(copies):
            for i in range(N_IMG):
                shutil.copy(os.path.join(root, 'train', kind, '%d.%s' % (i, ext)), os.path.join(dst, 'train', kind, '%d.%s' % (c * N_IMG + i, ext)))
    return dst


def test_the_loss_falls_through_the_driver(tmp_path, state, root, mano):
    """8 fixed images, augment=False: the mean total loss of the last 5 steps is below that of the first 5"""
    from dir_amd.apps import train as T
    data = replicate(root, str(tmp_path / 'data'), LOSS_STEPS)
    model = make_model(state)
    tb = train_batches(data, mano, bs=8, augment=False)
    res = T.fit(model, tb, None, output_root=str(tmp_path / 'out'), total_epoch=1, lr=LOSS_LR, step='graphed', print_iter=1, draw_iter=0,
                seed=SEED)
    totals = [t for _, t in res['printed']]
    print('total loss per step: ' + ' '.join('%.4g' % t for t in totals))
    assert len(totals) == LOSS_STEPS and all(np.isfinite(totals))
    assert np.mean(totals[-5:]) < np.mean(totals[:5]), (totals[:5], totals[-5:])


def test_iterations_that_do_not_print_do_not_synchronise(tmp_path, state, root, mano, monkeypatch):
    """--step graphed, print_iter 4, 8 iterations: 0 and 1 run eagerly (operand scales), 2 captures; 3, 5, 6 and 7 are replays that do not
    print -- no Tensor.item / cpu / tolist / __float__ / numpy, no torch.cuda.synchronize between one step's end and the next's (the input
    pipeline included); iteration 4 prints and reads the losses once."""
    from dir_amd.apps import train as T
    data = replicate(root, str(tmp_path / 'data'), 2)
    counts, cur = {}, [0]

    def counted(name, fn):
        def wrapper(*a, **k):
            counts.setdefault(cur[0], []).append(name)
            return fn(*a, **k)
        return wrapper
    for name in ('item', 'cpu', 'tolist', '__float__', '__int__', '__bool__', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, 'synchronize', counted('synchronize', torch.cuda.synchronize))
    model = make_model(state)

    def on_step(epoch, iteration, steps):
        cur[0] = iteration + 1                      # what follows belongs to the next iteration
    res = T.fit(model, train_batches(data, mano, bs=2), None, output_root=str(tmp_path / 'out'), total_epoch=1, lr=1e-5, step='graphed',
                print_iter=4, draw_iter=0, seed=SEED, max_steps=8, on_step=on_step)
    assert res['steps'] == 8 and [s for s, _ in res['printed']] == [1, 5]
    for it in (3, 5, 6, 7):
        assert not counts.get(it), (it, counts.get(it))
    assert counts.get(4) and len([c for c in counts[4] if c == 'cpu']) == 1, counts.get(4)
