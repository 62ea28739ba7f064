"""GPU: gradient clipping, non-finite step skipping and the averaged weights through the training driver (dir_amd.apps.train.fit, apps.eval
--ema), on the fake split and with the helpers of test_gpu_train_app.py (copied): batch size, step counts and learning rate are that file's.
Everything here is an equality of bits or of counters; no tolerance is used."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
from fake_train_split import write_train_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402

pytestmark = pytest.mark.gpu

N_IMG, BS, SEED = 8, 4, 3
GUARD = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)


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


def make_model(state):
    from dir_amd.models.dir import DIR
    m = DIR(21, 'unused', 0, compute_dtype=torch.float16)
    m.load_state_dict(state, strict=True)
    m.autotune = False
    return m.cuda()


def train_batches(root, mano, seed=SEED, bs=BS, **kw):
    from dir_amd.apps.trainset import TrainBatches
    return TrainBatches(root, mano, 'train', batch_size=bs, workers=2, seed=seed, **kw)


def val_batches(root, mano, bs=BS):
    from dir_amd.apps.trainset import TrainBatches
    return TrainBatches(root, mano, 'test', batch_size=bs, workers=2, seed=SEED, augment=False, shuffle=False)


def run_fit(state, root, mano, out, step, **kw):
    from dir_amd.apps import train as T
    model = make_model(state)
    args = dict(output_root=str(out), total_epoch=2, lr=1e-5, step=step, print_iter=0, draw_iter=0, seed=SEED)
    args.update(kw)
    res = T.fit(model, train_batches(root, mano), args.pop('val', None), **args)
    torch.cuda.synchronize()
    return model, res


def params_of(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def differing(a, b):
    return [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


def load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


def log_lines(out):
    return [l for l in open(os.path.join(str(out), 'log', 'train_DIR.log')).read().split('\n') if '[Epoch ' in l]


@pytest.fixture(scope='module')
def unflagged(tmp_path_factory, state, root, mano):
    """{step kind: the parameters after 3 steps of a fit with no flag}, each computed once"""
    cache = {}

    def get(step):
        if step not in cache:
            out = tmp_path_factory.mktemp('plain_' + step)
            model, res = run_fit(state, root, mano, out, step, max_steps=3)
            assert res['steps'] == 3 and not res['optimizer'].guarded
            cache[step] = (params_of(model), str(out))
        return cache[step]
    return get


@pytest.mark.parametrize('step', ['eager', 'graphed'])
def test_a_norm_bound_never_reached_changes_no_bit(tmp_path, state, root, mano, unflagged, step):
    want, plain_out = unflagged(step)
    model, res = run_fit(state, root, mano, tmp_path, step, max_steps=3, max_grad_norm=1e30)
    st = res['optimizer'].guard_stats()
    assert res['steps'] == 3 and (st['applied'], st['skipped'], st['clipped'], st['clip_coef']) == (3, 0, 0, 1.0) and st['grad_norm'] > 0
    assert not differing(want, params_of(model))
    assert sum(int(not torch.equal(want[k].cpu(), state[k])) for k in want) > len(want) // 2          # the steps did train
    # the files: four keys without the features, 'guard' with them ('ema' only with an average)
    assert sorted(load(os.path.join(plain_out, 'checkpoint', 'latest.pth'))) == ['last_epoch', 'net', 'optimizer', 'schedule']
    ck = load(os.path.join(str(tmp_path), 'checkpoint', 'latest.pth'))
    assert sorted(ck) == ['guard', 'last_epoch', 'net', 'optimizer', 'schedule'] and sorted(ck['optimizer']) == ['param_groups', 'state']


def poisoned_fit(state, root, mano, out, poison, **kw):
    """an eager fit whose optimizer.step sees a NaN in flat_grad on the (1-based) calls in `poison`; -> model, optimiser, parameters after
    every step, what fit returned or raised"""
    from dir_amd.apps import train as T
    model = make_model(state)
    opt = T.make_optimizer(model, 1e-5, skip_nonfinite=True)
    inner, calls, after = opt.step, [0], []

    def step():
        calls[0] += 1
        if calls[0] in poison:
            opt.flat_grad[opt.numel // 2] = float('nan')
        inner()
        after.append(params_of(model))
    opt.step = step
    args = dict(output_root=str(out), optimizer=opt, total_epoch=2, lr=1e-5, step='eager', draw_iter=0, seed=SEED, max_steps=3)
    args.update(kw)
    try:
        res = T.fit(model, train_batches(root, mano), None, **args)
    except T.NonFiniteLoss as e:
        res = e
    torch.cuda.synchronize()
    return model, opt, after, res


def test_a_poisoned_step_is_skipped_and_reported(tmp_path, state, root, mano):
    """print_iter 2 with two iterations per epoch: steps 1 and 3 print; step 2 is poisoned"""
    model, opt, after, res = poisoned_fit(state, root, mano, tmp_path, {2}, print_iter=2)
    assert isinstance(res, dict) and res['steps'] == 3 and len(after) == 3
    assert differing(after[0], {k: v.cuda() for k, v in state.items() if k in after[0]})           # step 1 trained
    assert not differing(after[0], after[1])                                                     # step 2 changed nothing
    assert differing(after[1], after[2])                                                         # step 3 trained again
    st = opt.guard_stats()
    assert (st['applied'], st['skipped'], st['skipped_in_row']) == (2, 1, 0)
    lines = log_lines(tmp_path)
    assert len(lines) == 2 and '[skipped 0]' in lines[0] and '[skipped 1]' in lines[1] and '[grad_norm ' in lines[1] and '[clip 1.0000]' in lines[1]
    assert lines[1].index('[loss_') < lines[1].index('[grad_norm ') < lines[1].index('[clip ') < lines[1].index('[skipped ')


def test_skipping_every_step_stops_the_run_with_the_weights_untouched(tmp_path, state, root, mano):
    from dir_amd.apps import train as T
    model, opt, after, res = poisoned_fit(state, root, mano, tmp_path, {1, 2, 3}, print_iter=2)
    assert isinstance(res, T.NonFiniteLoss) and 'skipped' in str(res)
    assert len(after) == 1                                                                       # raised on the first printing iteration
    assert not differing(after[0], {k: v.cuda() for k, v in state.items() if k in after[0]})
    assert torch.isfinite(opt.exp_avg).all() and not opt.exp_avg.any() and opt.guard_stats()['applied'] == 0


@pytest.mark.parametrize('decay', [0.0, 1.0])
def test_validation_judges_the_average(tmp_path, state, root, mano, decay):
    """decay 0: the average IS the raw weights, so validation inside fit equals validation of the model afterwards, bit for bit in every
    number.  decay 1: the average stays at the initial weights, so validation equals that of the initial parameters -- with the BatchNorm
    statistics of the trained model, since buffers are not averaged."""
    from dir_amd.apps import train as T
    vb = val_batches(root, mano)
    model, res = run_fit(state, root, mano, tmp_path, 'eager', ema_decay=decay, val=vb, total_epoch=1, lr=1e-4)
    assert res['last_val']['batches'] == 2 and np.isfinite(res['last_val']['error'])
    ck = load(os.path.join(str(tmp_path), 'checkpoint', 'best.pth'))
    assert sorted(ck) == ['ema', 'guard', 'last_epoch', 'net', 'optimizer', 'schedule'] and sorted(ck['ema']) == sorted(ck['net'])
    trained = [k for k in ck['net'] if not is_buf(k) and not torch.equal(ck['net'][k], state[k])]
    assert len(trained) > len(ck['net']) // 2
    assert not differing({k: v for k, v in ck['net'].items() if not is_buf(k)}, {k: v.cpu() for k, v in params_of(model).items()})      # raw weights are back
    if decay == 0.0:
        assert not [k for k in ck['net'] if not torch.equal(ck['net'][k], ck['ema'][k])]
        assert res['last_val'] == T.validate(model, vb, quiet=True)
    else:
        assert not [k for k in ck['ema'] if not torch.equal(ck['ema'][k], ck['net'][k] if is_buf(k) else state[k])]
        start = make_model(state)
        start.load_state_dict({k: (v if is_buf(k) else state[k]) for k, v in ck['net'].items()}, strict=True)
        assert res['last_val'] == T.validate(start, vb, quiet=True)
        assert res['last_val'] != T.validate(model, vb, quiet=True)


@pytest.fixture(scope='module')
def guarded_runs(tmp_path_factory, state, root, mano):
    """an uninterrupted two-epoch run with all three features on, and the same run stopped after epoch 0 and resumed.  The f16x3 operand
    scales of the training convolutions (dir_amd.train.conv) are measured on an optimiser's first step and kept for RECALIBRATE steps, so a
    resumed run measures them on the batch it starts with: with RECALIBRATE = 2 the uninterrupted run measures on steps 1 and 3, which is
    where the two halves measure, and the runs can be compared bit for bit."""
    from dir_amd.train import conv as TC
    whole, parts = tmp_path_factory.mktemp('whole'), tmp_path_factory.mktemp('parts')
    keep, TC.RECALIBRATE = TC.RECALIBRATE, 2
    try:
        _, res_w = run_fit(state, root, mano, whole, 'eager', **GUARD)
        _, first = run_fit(state, root, mano, parts, 'eager', max_steps=2, **GUARD)
        latest = os.path.join(str(parts), 'checkpoint', 'latest.pth')
        mid = load(latest)
        _, second = run_fit(state, root, mano, parts, 'eager', continue_train=latest, **GUARD)
    finally:
        TC.RECALIBRATE = keep
    return {'whole': load(os.path.join(str(whole), 'checkpoint', 'latest.pth')), 'mid': mid, 'resumed': load(latest), 'path': latest,
            'steps': (res_w['steps'], first['steps'], second['steps'])}


def test_resume_continues_the_uninterrupted_run_bit_for_bit(guarded_runs):
    a, b, mid = guarded_runs['whole'], guarded_runs['resumed'], guarded_runs['mid']
    assert guarded_runs['steps'] == (4, 2, 2) and mid['last_epoch'] == 0 and a['last_epoch'] == b['last_epoch'] == 1
    for ck in (a, b, mid):
        assert sorted(ck) == ['ema', 'guard', 'last_epoch', 'net', 'optimizer', 'schedule']
    assert mid['guard']['applied'] == 2 and a['guard'] == b['guard'] and a['guard']['applied'] == 4 and a['guard']['skipped'] == 0
    assert {k: a['guard'][k] for k in GUARD} == GUARD
    for key in ('net', 'ema'):
        assert sorted(a[key]) == sorted(b[key])
        bad = [k for k in a[key] if not torch.equal(a[key][k], b[key][k])]
        assert not bad, (key, len(bad), bad[:5])
    assert [k for k in a['net'] if not is_buf(k) and not torch.equal(a['net'][k], a['ema'][k])]            # the average lags
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sorted(sa) == sorted(sb) and all(float(s['step']) == 4.0 for s in sa.values())
    for i in sa:
        assert torch.equal(sa[i]['exp_avg'], sb[i]['exp_avg']) and torch.equal(sa[i]['exp_avg_sq'], sb[i]['exp_avg_sq']), i
    from dir_amd.models.dir import DIR
    DIR(21, 'unused', 0).load_state_dict(a['ema'], strict=True)                                            # 'ema' loads into DIR directly


def test_eval_app_loads_the_average_or_says_that_there_is_none(tmp_path, guarded_runs, unflagged, root):
    from dir_amd.apps import checkpoint_weights
    from dir_amd.apps import eval as E
    ck = guarded_runs['resumed']
    assert checkpoint_weights(ck, True) is ck['ema'] and checkpoint_weights(ck, False) is ck['net'] and checkpoint_weights(ck['net']) is ck['net']
    args = ['--data_path', root, '--bs', '4', '--workers', '2']
    ema = E.main(['--model', guarded_runs['path'], '--ema', '--result_dir', str(tmp_path / 'ema')] + args).summarize()
    raw = E.main(['--model', guarded_runs['path'], '--result_dir', str(tmp_path / 'raw')] + args).summarize()
    assert np.isfinite(ema['joint_mm']['all']) and np.isfinite(raw['joint_mm']['all']) and ema != raw
    plain = os.path.join(unflagged('eager')[1], 'checkpoint', 'latest.pth')
    with pytest.raises(KeyError, match='no averaged weights'):
        E.main(['--model', plain, '--ema', '--result_dir', str(tmp_path / 'none')] + args)


def replicate(root, dst, copies):
    for kind, ext in (('img', 'jpg'), ('mask', 'jpg'), ('dense', 'jpg'), ('anno', 'pkl')):
        os.makedirs(os.path.join(dst, 'train', kind), exist_ok=True)
        for c in range(copies):
            for i in range(N_IMG):
                shutil.copy(os.path.join(root, 'train', kind, '%d.%s' % (i, ext)), os.path.join(dst, 'train', kind, '%d.%s' % (c * N_IMG + i, ext)))
    return dst


def test_iterations_that_do_not_print_do_not_synchronise_with_the_flags_on(tmp_path, state, root, mano, monkeypatch):
    """test_gpu_train_app.py's method with all three features on: --step graphed, print_iter 4, 8 iterations; 3, 5, 6 and 7 are replays that
    do not print -- no Tensor.item / cpu / tolist / __float__ / numpy, no torch.cuda.synchronize; iteration 4 prints and reads twice (the
    losses, the guard's state)."""
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
        cur[0] = iteration + 1
    res = T.fit(model, train_batches(data, mano, bs=2), None, output_root=str(tmp_path / 'out'), total_epoch=1, lr=1e-5, step='graphed',
                print_iter=4, draw_iter=0, seed=SEED, max_steps=8, on_step=on_step, **GUARD)
    assert res['steps'] == 8 and [s for s, _ in res['printed']] == [1, 5]
    for it in (3, 5, 6, 7):
        assert not counts.get(it), (it, counts.get(it))
    assert counts.get(4) and len([c for c in counts[4] if c == 'cpu']) == 2, counts.get(4)
    lines = log_lines(tmp_path / 'out')
    assert len(lines) == 2 and all('[skipped 0]' in l for l in lines)
