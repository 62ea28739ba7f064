"""GPU: dir_mano_fit (csrc/mano_fit.hip) -- MANO parameters fitted to meshes, 3-D joints and 2-D keypoints inside one launch -- against the
float64 restatement of its rule (tests/helpers/mano_fit_ref.py), and the Python surface on top of it (utils/mano_fit.py, apps/fit_mano.py,
apps/predict.py --keypoints).

Gates: |kernel - float64 restatement| <= 4 x the largest |float32 restatement - float64 restatement| that tests/test_mano_fit_ref.py measured on
the CPU for that configuration, iteration count and output (mano_fit_ref.GATES); nothing here is measured on the kernel.  Every figure is printed
before it is asserted.

Hostile rows: lr 1e3 on its own does not overflow (Adam's steps are lr-sized whatever the gradient: the float32 restatement stays below 1.4e4
over 50 steps), so the row that must end with status bit 2 also gets w_verts 1e20, at which the second step's v overflows (restatement: one step
taken; 1e18 does not overflow, 1e22 overflows at once).

Measured on the MI355X (information, not a bound): the kernel used 0.03 .. 0.37 of its gates over the three configurations x 1, 2, 10, 50 iterations x
both hands; cold start 24 .. 43 mm -> at most 0.0032 mm; refinement 7.72 x (right), 9.75 x (left); predict's keypoints shifted by 3.6 px: 0.14 .. 0.18 px left
after 50 steps.  Every bit equality held; the degenerate 6D starts ended with status 0, 4, 4 and finite parameters."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import mano_fit_ref as R  # noqa: E402
import mano_gpu_run as G  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd import functional as F  # noqa: E402
from dir_amd.utils import mano_fit as MF  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after', 'status')
_REF = {}


def ref64(config, side, iters):
    """the float64 restatement on problem(config, 3, side): computed once, shared, not to be written to"""
    key = (config, side, iters)
    if key not in _REF:
        _REF[key] = R.fit(R.problem(config, 3, side), iters, torch.float64)
    return _REF[key]


def tables(prob):
    return G.packed(R.KIND, prob.side, prob.center, prob.root_palm)


def dev(a, rows=None):
    if a is None:
        return None
    a = np.asarray(a, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).cuda()


def run(probs, iters, rows=None, state=None, anchor=None, init=None, lr=None, weights=None, outputs=True):
    """fit_mano on one Problem (one hand) or a list of two (a pair); rows: the rows of the problem to take -> FitResult of device tensors"""
    pair = not isinstance(probs, R.Problem)
    ps = list(probs) if pair else [probs]
    arg = lambda k: [dev(getattr(p, k), rows) for p in ps] if pair else dev(getattr(ps[0], k), rows)  # noqa: E731
    p0 = arg('init') if init is None else init
    lr4 = ps[0].lr if lr is None else lr
    return MF.fit_mano([tables(p) for p in ps] if pair else tables(ps[0]), p0, arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'),
                       iters=iters, lr=dict(zip(MF.GROUPS, lr4)), weights=ps[0].weights if weights is None else weights, state=state, outputs=outputs, anchor=anchor)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, fields=FIELDS):
    return all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in fields)


def hand(res, h):
    return MF.FitResult(*[None if f is None else f[h] for f in res])


def forward_bits(prob, para):
    """dir_mano_forward at para [B,64] with the problem's tables -> verts, joints, joint_uv"""
    B = para.shape[0]
    v, j, u = torch.empty(B, 778, 3, device='cuda'), torch.empty(B, 21, 3, device='cuda'), torch.empty(B, 21, 2, device='cuda')
    base = para.data_ptr()
    import ctypes as C
    _capi.check(_capi.lib().dir_mano_forward(tables(prob), C.c_void_p(base), 64, C.c_void_p(base + 51 * 4), 64, C.c_void_p(base + 61 * 4), 64, _capi.ptr(v), _capi.ptr(j),
                                             _capi.ptr(u), None, None, B, _capi.stream_ptr()), 'dir_mano_forward')
    return v, j, u


def test_zero_iterations_are_the_forward():
    """iters = 0: para = init bit for bit, the outputs are dir_mano_forward's bits, mse_before == mse_after; B 1, 2, 3 x 1 and 2 hands; root_palm too"""
    for config in ('mesh', 'joints', 'uv'):
        for B in (1, 2, 3):
            pl, pr = R.problem(config, 3, 'left'), R.problem(config, 3, 'right', root_palm=(config == 'joints'))
            rows = list(range(B))
            single, pair = run(pr, 0, rows), run([pl, pr], 0, rows)
            torch.cuda.synchronize()
            for res, prob in ((single, pr), (hand(pair, 0), pl), (hand(pair, 1), pr)):
                init = dev(prob.init, rows)
                assert torch.equal(bits(res.para), bits(init)) and res.status.tolist() == [0] * B
                for got, want in zip((res.verts, res.joints, res.joint_uv), forward_bits(prob, init)):
                    assert torch.equal(bits(got), bits(want)), (config, B, prob.name)
                assert torch.equal(bits(res.mse_before), bits(res.mse_after))
                k = {'mesh': 0, 'joints': 1, 'uv': 2}[config]
                assert bool((res.mse_before[:, k] > 0).all()) and float(res.mse_before.sum()) == float(res.mse_before[:, k].sum())


@pytest.mark.parametrize('config', ['mesh', 'joints', 'uv'])
def test_trajectory_parity_with_the_float64_restatement(config):
    """iters 1, 2, 10, 50, both hands in one launch (B = 3 x 2 hands): V, J, U at the fitted p, mse_after and p itself inside 4 x the CPU-recorded
    float32-against-float64 differences"""
    pl, pr = R.problem(config, 3, 'left'), R.problem(config, 3, 'right')
    worst = {}
    for it in R.ITERS:
        pair = run([pl, pr], it)
        torch.cuda.synchronize()
        for h, side in enumerate(('left', 'right')):
            ref, got = ref64(config, side, it), hand(pair, h)
            assert got.status.tolist() == ref['status'].tolist() == [0, 0, 0]
            for k in R.OUTPUTS:
                d = float((getattr(got, k).double().cpu() - ref[k]).abs().max())
                worst[(it, side, k)] = (d, R.gate(config, it, k))
    for key, (d, g) in sorted(worst.items()):
        print(config, key, 'difference %.3g gate %.3g (%.2f of it)' % (d, g, d / g))
    for key, (d, g) in worst.items():
        assert d <= g, (config, key, d, g)


def test_bit_equalities():
    """the left hand fits 2-D keypoints with the prior, the right hand a mesh, in one launch (one set of weights and rates serves both)"""
    pl, pr = R.problem('uv', 3, 'left'), R.problem('mesh', 3, 'right')
    W, LR = {'w_verts': 1e4, 'w_uv': 1.0, 'w_init': 1e-3}, (0.02, 0.02, 0.01, 0.02)
    both = lambda iters, probs=(pl, pr), **kw: run(list(probs), iters, lr=LR, weights=W, **kw)  # noqa: E731
    keep = lambda r: MF.FitResult(*[[None if t is None else t.clone() for t in f] for f in r])  # noqa: E731
    base = keep(both(10))
    torch.cuda.synchronize()
    assert all(not torch.equal(bits(base.para[h]), bits(dev(p.init))) for h, p in ((0, pl), (1, pr)))
    # a repeat run
    again = both(10)
    assert all(same(hand(base, h), hand(again, h)) for h in (0, 1))
    # a row alone (B = 1, one hand) against slot 2 of the batch of 3; hand slot 0 against hand slot 1
    for h, prob in ((0, pl), (1, pr)):
        alone = run(prob, 10, rows=[2], lr=LR, weights=W)
        assert all(torch.equal(bits(getattr(alone, k))[0], bits(getattr(hand(base, h), k))[2]) for k in FIELDS), prob.name
    swapped = both(10, (pr, pl))
    assert same(hand(swapped, 0), hand(base, 1)) and same(hand(swapped, 1), hand(base, 0))
    # iters 5 + 5 with the state against iters 10 (the prior stays centred on the first start)
    st10 = [MF.new_state(3), MF.new_state(3)]
    whole = both(10, state=st10)
    first = both(5, state=True)
    second = both(5, state=first.state, init=[t.clone() for t in first.para], anchor=[dev(pl.init), dev(pr.init)])
    fields = tuple(k for k in FIELDS if k != 'mse_before')
    assert all(same(hand(whole, h), hand(second, h), fields) and same(hand(whole, h), hand(base, h)) for h in (0, 1))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(st10, second.state))
    assert st10[0][:, 130].view(torch.int32).tolist() == [10, 10, 10]
    # para_out aliasing init
    p0 = [dev(pl.init), dev(pr.init)]
    tabs, t_uv, t_conf, t_verts = [tables(pl), tables(pr)], dev(pl.joint_uv), dev(pl.uv_conf), dev(pr.verts)
    call = lambda init, out=None: F.mano_fit(tabs, init, joint_uv=[t_uv, None], uv_conf=[t_conf, None], verts=[None, t_verts], iters=10, lr=LR, weights=W,  # noqa: E731
                                             para_out=out)
    al = call(p0, p0)
    assert al[0]['para'] is p0[0] and all(torch.equal(bits(p0[h]), bits(base.para[h])) for h in (0, 1))
    # a group with lr 0 keeps its bits while the others move
    for g, sl in zip(MF.GROUPS, R.GROUP_SLICES):
        r = run(pr, 10, lr=[0.0 if x == g else 0.02 for x in MF.GROUPS])
        moved = bits(r.para) != bits(dev(pr.init))
        assert not bool(moved[:, sl].any()), g
        assert all(bool(moved[:, s2].any()) for s2 in R.GROUP_SLICES[:3] if s2 != sl), g       # (a mesh target alone gives cam no gradient)
        assert not bool(moved[:, R.GROUP_SLICES[3]].any())
    # a captured graph replay against the eager launch
    init = [dev(pl.init), dev(pr.init)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(init)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(init)
    graph.replay()
    torch.cuda.synchronize()
    for h in (0, 1):
        for k in ('para', 'verts', 'joints', 'joint_uv', 'status'):
            assert torch.equal(bits(out[h][k]), bits(getattr(hand(base, h), k))), (h, k)
        assert torch.equal(bits(out[h]['mse']), bits(torch.cat([base.mse_before[h], base.mse_after[h]], 1)))


def test_hostile_rows():
    prob = R.problem('joints', 3, 'right')
    base = run(prob, 10)
    finite = lambda r: all(bool(torch.isfinite(getattr(r, k)).all()) for k in ('verts', 'joints', 'joint_uv', 'mse_before', 'mse_after'))  # noqa: E731
    assert np.isnan(prob.joints).any() and base.status.tolist() == [0, 0, 0] and finite(base) and bool(torch.isfinite(base.para).all())
    # NaN under confidence 0 = finite garbage there, bit for bit
    junk = prob.joints.copy()
    junk[np.isnan(junk)] = 12345.0
    assert same(base, run(prob._replace(joints=junk), 10))
    # NaN under confidence > 0, and NaN in init: bit 1, p0's bits back, the state unchanged; the other rows as before
    conf = prob.joints_conf.copy()
    conf[1][conf[1] == 0] = 0.5
    st = MF.new_state(3)
    st[:, :128] = 0.25
    keep = st.clone()
    r = run(prob._replace(joints_conf=conf), 10, state=st)
    assert r.status.tolist() == [0, 2, 0] and finite(r) and torch.equal(bits(r.para[1]), bits(dev(prob.init)[1]))
    assert torch.equal(bits(st[1]), bits(keep[1])) and not torch.equal(bits(st[0]), bits(keep[0])) and float(r.mse_after[1].abs().max()) == 0.0
    bad = prob.init.copy()
    bad[2, 30] = np.nan
    bad[0, 3] = np.inf
    st = MF.new_state(3)
    r = run(prob._replace(init=bad), 10, state=st)
    assert r.status.tolist() == [2, 0, 2] and finite(r) and torch.equal(bits(r.para), bits(torch.where(torch.tensor([True, False, True], device='cuda')[:, None], dev(bad), base.para)))
    assert float(st[0].abs().max()) == 0.0 and float(st[2].abs().max()) == 0.0 and float(r.verts[0].abs().max()) == 0.0
    assert torch.equal(bits(r.verts[1]), bits(base.verts[1]))
    # lr 1e3 (+ w_verts 1e20, see the module docstring): a step goes non-finite, bit 2, the last finite iterate comes back
    hot = R.problem('mesh', 3, 'left')
    st = MF.new_state(3)
    r = run(hot, 10, lr=(1e3,) * 4, weights=dict(hot.weights, w_verts=1e20), state=st)
    print('lr 1e3, w_verts 1e20: status', r.status.tolist(), 'steps taken', st[:, 130].view(torch.int32).tolist(), 'max |p| %.4g' % float(r.para.abs().max()))
    assert all(s & 4 for s in r.status.tolist()) and bool(torch.isfinite(r.para).all()) and finite(r) and bool(torch.isfinite(st[:, :130]).all())
    assert all(0 <= t < 10 for t in st[:, 130].view(torch.int32).tolist())
    # exactly parallel and zero 6D columns: finite outputs or bit 1, never a non-finite p
    deg = R.problem('mesh', 3, 'right')
    init = deg.init.copy()
    init[0, 3:6] = init[0, 0:3]
    init[1, 0:3] = 0.0
    init[2, 0:6] = 0.0
    r = run(deg._replace(init=init), 10)
    print('degenerate 6D starts: status', r.status.tolist())
    assert bool(torch.isfinite(r.para).all())
    for b, s in enumerate(r.status.tolist()):
        assert (s & 2) or all(bool(torch.isfinite(getattr(r, k)[b]).all()) for k in ('verts', 'joints', 'joint_uv')), (b, s)


def test_convergence_on_the_gpu():
    """cold start on mesh targets, 200 iterations at lr 0.1: every sample's vertex RMS below 1 mm (the float64 restatement reaches 0.003 mm on these
    hands); the refinement case, 100 iterations: the worst sample's 2-D RMS falls by at least 5 x (the restatement: 7.7 x right, 9.8 x left)"""
    for side in ('right', 'left'):
        cold = R.problem('mesh', 6, side)
        r = run(cold, 200, lr=(0.1,) * 4)
        rms = r.mse_after[:, 0].sqrt() * 1e3
        print(side, 'cold start vertex RMS mm: %s -> %s' % ((r.mse_before[:, 0].sqrt() * 1e3).tolist(), rms.tolist()))
        assert r.status.tolist() == [0] * 6 and float(rms.max()) < 1.0 and float((r.mse_before[:, 0].sqrt() * 1e3).min()) > 20.0
        direct = (r.verts - dev(cold.verts)).pow(2).sum(-1).mean(1).sqrt() * 1e3          # the residual, from the outputs themselves
        assert float(direct.max()) < 1.0
        ref = R.problem('uv', 6, side)
        r = run(ref, 100)
        before, after = r.mse_before[:, 2].sqrt(), r.mse_after[:, 2].sqrt()
        print(side, 'refinement 2-D RMS: %.4f -> %.4f (%.2f x)' % (float(before.max()), float(after.max()), float(before.max() / after.max())))
        assert float(before.max() / after.max()) >= 5.0
        assert torch.equal(bits(r.para[:, 51:61]), bits(dev(ref.init)[:, 51:61]))


def test_fit_mano_surface():
    """a ManoLayer as `layer_or_tables`, a pair given as lists, lr as a float, default weights, outputs=False, B = 0, bad arguments"""
    from dir_amd.manopth.manolayer import ManoLayer
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=R.CENTER, flat_hand_mean=False, side=s, seed=1234).cuda() for s in ('left', 'right')]
    pl, pr = R.problem('mesh', 2, 'left'), R.problem('mesh', 2, 'right')
    want = run([pl, pr], 5, lr=(0.05,) * 4, weights={'w_verts': 1e4})
    got = MF.fit_mano(layers, [dev(pl.init), dev(pr.init)], verts=[dev(pl.verts), dev(pr.verts)], iters=5, lr=0.05)
    assert all(same(hand(want, h), hand(got, h)) for h in (0, 1))
    lean = MF.fit_mano(layers[1], dev(pr.init), verts=dev(pr.verts), iters=5, lr=0.05, outputs=False)
    assert lean.verts is None and torch.equal(bits(lean.para), bits(got.para[1])) and lean.state is None
    cold = MF.neutral_para(2, 4.0)
    assert torch.equal(cold.cpu(), R.neutral_para(2, 4.0).float())
    empty = MF.fit_mano(layers[1], torch.empty(0, 64, device='cuda'), verts=torch.empty(0, 778, 3, device='cuda'), iters=5)
    assert empty.para.shape == (0, 64) and empty.status.shape == (0,)
    with pytest.raises(ValueError):
        MF.fit_mano(layers[1], dev(pr.init), verts=dev(pr.verts), lr={'wrist': 0.1})
    with pytest.raises(_capi.DirHipError):
        MF.fit_mano(layers[1], dev(pr.init), verts=dev(pr.verts)[:, :700])
    with pytest.raises(_capi.DirHipError):
        MF.fit_mano(layers[1], dev(pr.init), verts=dev(pr.verts), iters=-1)


# ===================================================================================================================== the commands
@pytest.fixture(scope='module')
def state():
    from dir_amd import synth
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def test_fit_mano_command_round_trip(tmp_path, state, capsys):
    """apps.fit_mano on the fake split's ground-truth meshes, root-relative (the wrist is joint 0 of both layers): the npz fields, residuals that fall
    from centimetres to well under the convergence test's millimetre, and para_<side> that dir_mano_forward turns back into the fitted meshes"""
    from fake_split import write_split

    from dir_amd.apps import dataset as DS
    from dir_amd.apps import fit_mano as A
    root = str(tmp_path / 'split')
    write_split(root, 5, seed=3)
    ds = DS.InterHandSplit(root)
    annos = torch.from_numpy(np.stack([ds.anno(i) for i in range(5)])).cuda()
    jl, vl, jr, vr = DS.gt_batch(DS.gt_layers_from_checkpoint(state), annos)[:4]
    tg = {'verts_left': (vl - jl[:, :1]).cpu().numpy(), 'verts_right': (vr - jr[:, :1]).cpu().numpy()}
    np.savez(str(tmp_path / 'T.npz'), **tg)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    n = A.main(['--model', ck, '--targets', str(tmp_path / 'T.npz'), '--out', str(tmp_path / 'O.npz'), '--iters', '200', '--lr', '0.1', '--bs', '3'])
    assert n == 10 and capsys.readouterr().out.strip().splitlines()[-1].startswith('10 hands in ')
    out = np.load(str(tmp_path / 'O.npz'))
    assert sorted(out.files) == sorted('%s_%s' % (k, s) for s in ('left', 'right') for k in FIELDS)
    tabs, keep = A.tables_from_checkpoint(state, 0)
    for s in ('left', 'right'):
        before, after = np.sqrt(out['mse_before_' + s][:, 0]) * 1e3, np.sqrt(out['mse_after_' + s][:, 0]) * 1e3
        print(s, 'vertex RMS mm', before.tolist(), '->', after.tolist())
        assert out['para_' + s].shape == (5, 64) and out['status_' + s].tolist() == [0] * 5
        assert before.min() > 5.0 and after.max() < 2.0 and (after < before / 20.0).all()
        assert np.abs(np.sqrt(((out['verts_' + s] - tg['verts_' + s]) ** 2).sum(-1).mean(1)) * 1e3 - after).max() < 1e-3
        v, j, u = (t.cpu().numpy() for t in forward_bits_tables(tabs[s], torch.from_numpy(out['para_' + s]).cuda()))
        assert np.array_equal(v, out['verts_' + s]) and np.array_equal(j, out['joints_' + s]) and np.array_equal(u, out['joint_uv_' + s]), s


def forward_bits_tables(T, para):
    import ctypes as C
    B = para.shape[0]
    v, j, u = torch.empty(B, 778, 3, device='cuda'), torch.empty(B, 21, 3, device='cuda'), torch.empty(B, 21, 2, device='cuda')
    base = para.data_ptr()
    _capi.check(_capi.lib().dir_mano_forward(T, C.c_void_p(base), 64, C.c_void_p(base + 51 * 4), 64, C.c_void_p(base + 61 * 4), 64, _capi.ptr(v), _capi.ptr(j),
                                             _capi.ptr(u), None, None, B, _capi.stream_ptr()), 'dir_mano_forward')
    return v, j, u


@pytest.fixture(scope='module')
def eng(state):
    from dir_amd.engine import DirEngine
    return DirEngine(state, dtype=torch.float16)


def test_predict_with_keypoints(tmp_path, state, eng):
    """predict(keypoints=...) on the fake split's frames (box = the frame: the crop is the frame); the keypoints are the network's own 2-D joints
    shifted by (3, -2) px, the right hand of frame 1 and all of frame 3 have none.  The refined 2-D joints lie closer to the keypoints by at least
    half the reduction the float64 restatement reaches on the same inputs (the checkpoint's MANO tables are synth.mano_buffers(side, 1234), which
    are mano_cases' 'pca' tables); "unrefined" is the unflagged run bit for bit; a hand with no keypoints passes through bit for bit."""
    from fake_split import write_split

    from dir_amd.apps import dataset as DS
    from dir_amd.apps import predict as P
    from dir_amd.utils import crop as CR
    root = str(tmp_path / 'split')
    write_split(root, 4, seed=5)
    ds = DS.InterHandSplit(root)
    frames = [np.ascontiguousarray(ds.frame(i)) for i in range(4)]
    boxes = [[0, 0, 256, 256]] * 4
    plain = P.predict(eng, frames, boxes, ratio=1.0, stage=2, bs=4, keep_stage=True)
    assert all(r['matrix'] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]] for r in plain)
    shift = np.float32([3.0, -2.0])
    kps = []
    for i, r in enumerate(plain):
        e = {s: np.concatenate([np.float32(r[s]['joints_px']) + shift, np.ones((21, 1), np.float32)], 1).tolist() for s in P.SIDES}
        if i == 1:
            del e['right']
        kps.append(None if i == 3 else e)
    got = P.predict(eng, frames, boxes, ratio=1.0, stage=2, bs=4, keep_stage=True, keypoints=kps)
    again = P.predict(eng, frames, boxes, ratio=1.0, stage=2, bs=4, keep_stage=True)
    strip = lambda r: json.dumps({k: v for k, v in r.items() if not k.startswith('stage')}, sort_keys=True)  # noqa: E731
    assert [strip(x) for x in plain] == [strip(y) for y in again]
    # the restatement on the same inputs: the network's own stage-2 parameters, the keypoints in crop coordinates rounded once
    outs = eng.forward(torch.from_numpy(np.stack(frames)).cuda(), want_proj_feat=False, want_para=True)
    para = {s: outs[2]['pd_mano_para_' + s].float().cpu().numpy() for s in P.SIDES}
    eye = torch.tensor([[1.0, 0, 0, 0, 1.0, 0]] * 4, dtype=torch.float64)
    gain = {}
    for h, s in enumerate(P.SIDES):
        kp = P.keypoint_array(kps)[:, h]
        uv = CR.from_frame_pixels(torch.from_numpy(kp[:, :, :2]), eye, 256).float().numpy()
        prob = R.Problem('refine_' + s, s, 0, False, para[s], None, None, None, uv, kp[:, :, 2], dict(dict.fromkeys(R.WEIGHTS, 0.0), w_uv=1.0, w_init=1e-3),
                         (0.01, 0.01, 0.0, 0.01))
        ref = R.fit(prob, 50, torch.float64)
        gain[s] = (ref['mse_before'][:, 2].sqrt() - ref['mse_after'][:, 2].sqrt()).numpy() * 128.0           # px, per frame
    for i, (r, p) in enumerate(zip(got, plain)):
        assert r['refined'] is True and set(r['unrefined']) == set(P.SIDES)
        for s in P.SIDES:
            assert json.dumps(r['unrefined'][s], sort_keys=True) == json.dumps(p[s], sort_keys=True), (i, s)
            assert np.array_equal(r['stage_unrefined']['pd_mesh_xyz_' + s], p['stage']['pd_mesh_xyz_' + s])
            has = kps[i] is not None and s in kps[i]
            assert r['refined_hands'][s] == has
            if not has:
                assert json.dumps(r[s], sort_keys=True) == json.dumps(p[s], sort_keys=True)
                assert all(np.array_equal(r['stage'][k + s], p['stage'][k + s]) for k in ('pd_mesh_xyz_', 'pd_proj_', 'pd_joint_uv_'))
                continue
            target = np.float32(kps[i][s])[:, :2]
            d0 = np.sqrt(((np.float32(p[s]['joints_px']) - target) ** 2).sum(-1).mean())
            d1 = np.sqrt(((np.float32(r[s]['joints_px']) - target) ** 2).sum(-1).mean())
            print('frame %d %s: 2-D RMS to the keypoints %.3f px -> %.3f px (the restatement gains %.3f px)' % (i, s, d0, d1, gain[s][i]))
            assert abs(d0 - np.sqrt(13.0)) < 1e-3 and gain[s][i] > 0.5
            assert d0 - d1 >= 0.5 * gain[s][i], (i, s, d0, d1, gain[s][i])


def test_predict_command_with_and_without_keypoints(tmp_path, state, eng):
    """the unflagged command writes the same bytes before and after a --keypoints run in the same session; main(--keypoints) reads the JSON (by name
    and by stem, one image absent) and writes "unrefined" = the unflagged fields"""
    from fake_split import write_split
    from PIL import Image

    from dir_amd.apps import dataset as DS
    from dir_amd.apps import predict as P
    root = str(tmp_path / 'split')
    write_split(root, 3, seed=6)
    ds = DS.InterHandSplit(root)
    src = tmp_path / 'in'
    src.mkdir()
    names = ['a1.png', 'a2.png', 'a3.png']
    for i, n in enumerate(names):
        Image.fromarray(np.ascontiguousarray(ds.frame(i)[:, :, ::-1])).save(str(src / n), format='PNG')
    paths = [[str(src / n) for n in names]]

    def files(d):
        return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}
    P.run(eng, paths, str(tmp_path / 'A'), bs=2, workers=2)
    before = files(str(tmp_path / 'A'))
    recs = {n: json.loads(before[os.path.splitext(n)[0] + '.json']) for n in names}
    kp = {('a1.png', 'a2')[i]: {s: [[x + 2.0, y + 1.0, 0.9] for x, y in recs[n][s]['joints_px']] for s in P.SIDES} for i, n in enumerate(names[:2])}
    with open(tmp_path / 'kp.json', 'w') as f:
        json.dump(kp, f)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    assert P.main(['--model', ck, '--input', str(src), '--out', str(tmp_path / 'K'), '--bs', '2', '--workers', '2', '--keypoints', str(tmp_path / 'kp.json'),
                   '--refine_iters', '20']) == 3
    P.run(eng, paths, str(tmp_path / 'B'), bs=2, workers=2)
    assert files(str(tmp_path / 'B')) == before and sorted(before) == ['a1.json', 'a2.json', 'a3.json']
    flagged = files(str(tmp_path / 'K'))
    for i, n in enumerate(names):
        r, p = json.loads(flagged[os.path.splitext(n)[0] + '.json']), recs[n]
        assert r['refined'] is True and r['refined_hands'] == {s: i < 2 for s in P.SIDES}
        assert all(r['unrefined'][s] == p[s] for s in P.SIDES) and r['matrix'] == p['matrix'] and r['offset'] == p['offset']
        assert all((r[s] == p[s]) == (i == 2) for s in P.SIDES)
    with pytest.raises(SystemExit):
        P.main(['--model', ck, '--input', str(src), '--out', str(tmp_path / 'X'), '--refine_iters', '20'])
