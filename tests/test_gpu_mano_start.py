"""GPU: dir_mano_fit_start (csrc/mano_fit_start.hip) -- the closed-form start of a MANO fit: the root by a rigid alignment or a search over the cube's
24 rotations, the camera by least squares, in one launch -- against the float64 restatement of its rule (tests/helpers/mano_start_ref.py), and the
Python surface on top of it (utils/mano_fit.py start_mano, fit_mano(start='closed'), apps/fit_mano.py --start).

Gates: status and choice equal exactly; the root's angle, the camera and `info` (relative) within 4 x the largest |float32 restatement - float64
restatement| that tests/test_mano_start_ref.py measured on the CPU for that case (mano_start_ref.GATES); nothing here is gated on a figure taken from
the kernel.  Every figure is printed before it is asserted.

Measured on the MI355X (information, not a bound): the kernel used 0.13 .. 0.43 of its gates over the six cases x both hands (worst: root angle
4.1e-7 rad against 9.6e-7, root_palm); where a gate is 0 (the searched root, a camera no step touches) its value was the restatement's exactly; status
and choice equal everywhere.  Far meshes after 50 iterations at lr 0.1: 7.9 .. 23.1 mm cold, 0.82 .. 1.34 mm started.  The command, 20 iterations: 21 .. 41 mm
(meshes) and 11 .. 24 mm (joints) from the neutral start, 3.4 .. 5.7 mm and 2.3 .. 4.1 mm from the closed one.  Every bit equality held; the degenerate 6D
starts ended with status 0, 0, 16 and finite parameters."""
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
import mano_start_ref as S  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd import functional as F  # noqa: E402
from dir_amd.utils import mano_fit as MF  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ('para', 'status', 'choice', 'info')
TARGETS = ('verts', 'joints', 'joints_conf', 'joint_uv', 'uv_conf')
_CASE, _REF = {}, {}


def case(name, side, n=3):
    if (name, side, n) not in _CASE:
        _CASE[(name, side, n)] = S.case(name, side, n)
    return _CASE[(name, side, n)]


def ref64(name, side, n=3):
    """the float64 restatement on case(name, side, n): computed once, shared, not to be written to"""
    if (name, side, n) not in _REF:
        _REF[(name, side, n)] = S.start(case(name, side, n)[0], torch.float64)
    return _REF[(name, side, n)]


def tables(prob):
    return G.packed(S.KIND, prob.side, prob.center, prob.root_palm)


def dev(a, rows=None):
    if a is None:
        return None
    a = np.asarray(a, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).cuda()


def args_of(probs, rows=None):
    pair = not isinstance(probs, R.Problem)
    ps = list(probs) if pair else [probs]
    arg = lambda k: [dev(getattr(p, k), rows) for p in ps] if pair else dev(getattr(ps[0], k), rows)  # noqa: E731
    return ([tables(p) for p in ps] if pair else tables(ps[0])), arg('init'), [arg(k) for k in TARGETS]


def run(probs, rows=None, **kw):
    """start_mano on one Problem (one hand) or a list of two (a pair; the first one's weights serve both) -> StartResult of device tensors"""
    tabs, init, tg = args_of(probs, rows)
    w = (probs if isinstance(probs, R.Problem) else probs[0]).weights
    return MF.start_mano(tabs, init, *tg, weights=w, **kw)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, fields=FIELDS):
    return all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in fields)


def hand(res, h):
    return type(res)(*[None if f is None else f[h] for f in res])


def as_ref(res):
    return {'para': res.para.double().cpu(), 'info': res.info.double().cpu()}


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_parity_with_the_float64_restatement(name):
    """both hands in one launch, B = 3 x 2 hands: status and choice exactly, root angle / camera / info inside 4 x the CPU-recorded differences"""
    pl, pr = case(name, 'left')[0], case(name, 'right')[0]
    pair = run([pl, pr])
    torch.cuda.synchronize()
    worst = {}
    for h, (side, prob) in enumerate((('left', pl), ('right', pr))):
        got, ref = hand(pair, h), ref64(name, side)
        print(name, side, 'status', got.status.tolist(), 'choice', got.choice.tolist())
        assert got.status.tolist() == ref['status'].tolist() and got.choice.tolist() == ref['choice'].tolist()
        assert torch.equal(bits(got.para[:, 6:61]), bits(dev(prob.init)[:, 6:61]))
        for k, d in S.differences(as_ref(got), ref).items():
            worst[(side, k)] = (d, S.gate(name, k))
    for key, (d, g) in sorted(worst.items()):
        print(name, key, 'difference %.3g gate %.3g' % (d, g))
    for key, (d, g) in worst.items():
        assert d <= g, (name, key, d, g)


def test_bit_equalities():
    """the left hand starts from 2-D keypoints (the search), the right from a mesh with joints and keypoints, in one launch"""
    pl, pr = case('uv', 'left', 5)[0], case('all', 'right', 5)[0]
    pl = pl._replace(weights=pr.weights)
    keep = lambda r: type(r)(*[[t.clone() for t in f] for f in r])  # noqa: E731
    base = keep(run([pl, pr]))
    torch.cuda.synchronize()
    for h, p in ((0, pl), (1, pr)):
        p0 = dev(p.init)
        assert torch.equal(bits(base.para[h][:, 6:61]), bits(p0[:, 6:61]))                      # PCA coefficients and betas
        assert not bool((bits(base.para[h][:, :6]) == bits(p0[:, :6])).all(1).any()) and not bool((bits(base.para[h][:, 61:]) == bits(p0[:, 61:])).all(1).any())
        assert base.status[h].tolist() == [0] * 5
    assert base.choice[1].tolist() == [-1] * 5 and all(0 <= k < 24 for k in base.choice[0].tolist())
    # a repeat of the same call
    again = run([pl, pr])
    assert all(same(hand(base, h), hand(again, h)) for h in (0, 1))
    # a row alone (B = 1, one hand) against slot 3 of the batch of 5; hands = 1 against half of hands = 2; hand slot 0 against hand slot 1
    for h, prob in ((0, pl), (1, pr)):
        alone = run(prob, rows=[3])
        assert all(torch.equal(bits(getattr(alone, k))[0], bits(getattr(hand(base, h), k))[3]) for k in FIELDS), prob.name
        assert same(run(prob), hand(base, h)), prob.name
    swapped = run([pr, pl])
    assert same(hand(swapped, 0), hand(base, 1)) and same(hand(swapped, 1), hand(base, 0))
    # the switches leave their groups' bits
    for h, prob in ((0, pl), (1, pr)):
        p0, full = dev(prob.init), hand(base, h)
        nr, nc, ns = run(prob, root=False), run(prob, cam=False), run(prob, search=False)
        assert torch.equal(bits(nr.para[:, :6]), bits(p0[:, :6])) and torch.equal(bits(nc.para[:, 61:]), bits(p0[:, 61:]))
        if h == 0:                # 2-D alone: the search writes root and camera together; without it (or without `root`) only the camera may move
            want = S.start(prob, torch.float64, search=False)
            assert torch.equal(bits(nc.para), bits(p0)) and nc.choice.tolist() == [-1] * 5 and nc.status.tolist() == [0] * 5
            for r in (nr, ns):
                assert torch.equal(bits(r.para[:, :6]), bits(p0[:, :6])) and r.choice.tolist() == [-1] * 5 and r.status.tolist() == want['status'].tolist()
                assert same(r, nr)
        else:
            assert torch.equal(bits(nc.para[:, :6]), bits(full.para[:, :6])) and same(ns, full)
            assert nr.status.tolist() == S.start(prob, torch.float64, root=False)['status'].tolist() and nr.choice.tolist() == [-1] * 5
    # p_out aliasing p0
    tabs, init, tg = args_of([pl, pr])
    call = lambda p, out=None: F.mano_fit_start(tabs, p, *tg, w_verts=pr.weights['w_verts'], w_joints=pr.weights['w_joints'], para_out=out)  # noqa: E731
    al = call(init, init)
    assert al[0]['para'] is init[0] and all(torch.equal(bits(init[h]), bits(base.para[h])) for h in (0, 1))
    # a captured graph replay against the eager launch
    _, init, _ = args_of([pl, pr])
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
        for k in FIELDS:
            assert torch.equal(bits(out[h][k]), bits(getattr(hand(base, h), k))), (h, k)


def test_pass_through_and_hostile_rows():
    """hostile rows are ordinary inputs: NaN targets, NaN parameters, zero confidences, coincident keypoints, parallel and zero 6D columns"""
    prob = case('all', 'right')[0]
    base, p0 = run(prob), dev(prob.init)
    # NaN under confidence 0 = finite garbage there, bit for bit
    junk = prob.joint_uv.copy()
    assert np.isnan(junk).any()
    junk[np.isnan(junk)] = 12345.0
    assert same(base, run(prob._replace(joint_uv=junk)))
    # row 1: a NaN vertex; then a NaN keypoint under a confidence > 0; then NaN / inf in p0 -- the row passes through, the others are as before
    v = prob.verts.copy()
    v[1, 300, 2] = np.nan
    uc = prob.uv_conf.copy()
    uc[1][uc[1] == 0] = 0.5
    bad = prob.init.copy()
    bad[1, 30] = np.nan
    for p in (prob._replace(verts=v), prob._replace(uv_conf=uc), prob._replace(init=bad)):
        r, q0 = run(p), dev(p.init)
        assert r.status.tolist() == [0, 2, 0] and r.choice.tolist() == [-1] * 3 and float(r.info[1].abs().max()) == 0.0
        assert torch.equal(bits(r.para[1]), bits(q0[1]))
        assert all(torch.equal(bits(getattr(r, k)[[0, 2]]), bits(getattr(base, k)[[0, 2]])) for k in FIELDS)
    inf = prob.init.copy()
    inf[:, 61] = np.inf
    r = run(prob._replace(init=inf))
    assert r.status.tolist() == [2, 2, 2] and torch.equal(bits(r.para), bits(dev(inf)))
    # every confidence 0 (all targets NaN there), no vertices: nothing to align to and nothing to fit -> 8 | 16, p0's bits
    jp = case('root_palm', 'left')[0]
    z = np.zeros((3, 21), np.float32)
    r = run(jp._replace(joints=np.full((3, 21, 3), np.nan, np.float32), joints_conf=z, joint_uv=np.full((3, 21, 2), np.nan, np.float32), uv_conf=z))
    assert r.status.tolist() == [24, 24, 24] and torch.equal(bits(r.para), bits(dev(jp.init))) and float(r.info.abs().max()) == 0.0
    sp = case('uv', 'left')[0]
    r = run(sp._replace(joint_uv=np.full((3, 21, 2), np.nan, np.float32), uv_conf=z))
    assert r.status.tolist() == [24, 24, 24] and r.choice.tolist() == [-1] * 3 and torch.equal(bits(r.para), bits(dev(sp.init)))
    # all keypoints at one position: the scale is 0, never accepted -> the camera (and, in the search, the root) stays
    flat = np.broadcast_to(np.float32([0.25, -0.5]), (3, 21, 2)).copy()
    r = run(sp._replace(joint_uv=flat))
    assert r.status.tolist() == [24, 24, 24] and torch.equal(bits(r.para), bits(dev(sp.init)))
    r = run(jp._replace(joint_uv=flat))
    assert r.status.tolist() == [16, 16, 16] and torch.equal(bits(r.para[:, 61:]), bits(dev(jp.init)[:, 61:])) and not torch.equal(bits(r.para[:, :6]), bits(dev(jp.init)[:, :6]))
    # exactly parallel and zero 6D columns: a pass-through, or finite parameters
    deg = prob.init.copy()
    deg[0, 3:6] = deg[0, 0:3]
    deg[1, 0:3] = 0.0
    deg[2, 0:6] = 0.0
    r = run(prob._replace(init=deg))
    print('degenerate 6D starts: status', r.status.tolist())
    assert bool(torch.isfinite(r.para).all()) and bool(torch.isfinite(r.info).all())
    for b, s in enumerate(r.status.tolist()):
        assert not (s & 3) or torch.equal(bits(r.para[b]), bits(dev(deg)[b]))


def test_composition_with_the_fit():
    """fit_mano(start='closed') = start_mano, then fit_mano(init = anchor = its parameters), bit for bit; one hand and a pair; start=None as before"""
    pl, pr = case('joints', 'left')[0], case('joints', 'right')[0]
    for probs in (pr, [pl, pr]):
        tabs, init, tg = args_of(probs)
        kw = dict(iters=5, lr=0.05, weights=pr.weights)
        st = MF.start_mano(tabs, init, *tg, weights=pr.weights)
        want = MF.fit_mano(tabs, st.para, *tg, anchor=st.para, **kw)
        got = MF.fit_mano(tabs, init, *tg, start='closed', **kw)
        plain, none = MF.fit_mano(tabs, init, *tg, **kw), MF.fit_mano(tabs, init, *tg, start=None, **kw)
        flat = lambda r: [t for f in r if f is not None for t in (f if isinstance(f, list) else [f]) if t is not None]  # noqa: E731
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(got), flat(want))) and len(flat(got)) == len(flat(want))
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(plain), flat(none)))
        assert not torch.equal(bits(flat(got)[0]), bits(flat(plain)[0]))
    with pytest.raises(ValueError):
        MF.fit_mano(tables(pr), dev(pr.init), joints=dev(pr.joints), start='warm')
    empty = MF.start_mano(tables(pr), torch.empty(0, 64, device='cuda'), joints=torch.empty(0, 21, 3, device='cuda'))
    assert empty.para.shape == (0, 64) and empty.status.shape == (0,) and empty.info.shape == (0, 4)
    with pytest.raises(_capi.DirHipError):
        MF.start_mano(tables(pr), dev(pr.init), joints=dev(pr.joints)[:, :20])
    with pytest.raises(_capi.DirHipError):
        MF.start_mano(tables(pr), dev(pr.init), joints=dev(pr.joints), weights={'w_joints': -1.0})


def test_far_meshes_end_to_end():
    """the far mesh case (root 1.8 .. 3.1 rad from the start), 50 iterations at lr 0.1: the kernel-started fit's vertex RMS is below the cold fit's on
    every row (float64 restatement on the CPU: about 1 mm against 8 .. 16 mm)"""
    for side in ('right', 'left'):
        prob = case('mesh', side, 4)[0]
        tabs, init, tg = args_of(prob)
        kw = dict(iters=50, lr=0.1, weights=prob.weights)
        cold, started = MF.fit_mano(tabs, init, *tg, **kw), MF.fit_mano(tabs, init, *tg, start='closed', **kw)
        c, s = cold.mse_after[:, 0].sqrt() * 1e3, started.mse_after[:, 0].sqrt() * 1e3
        print(side, 'vertex RMS mm after 50 iterations: cold', c.tolist(), 'started', s.tolist())
        assert started.status.tolist() == [0] * 4 and bool((s < c).all())


# ===================================================================================================================== the command
@pytest.fixture(scope='module')
def state():
    from dir_amd import synth
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def test_fit_mano_command_with_a_closed_start(tmp_path, state):
    """apps.fit_mano --start closed on 4 far hands a side (the checkpoint's MANO tables are the 'pca' tables of the cases): the new keys, para_<side> = the
    library call's, and a run without the flag = --start neutral, array for array"""
    from dir_amd.apps import fit_mano as A
    pl, pr = case('mesh', 'left', 4)[0], case('joints', 'right', 4)[0]
    tg = {'verts_left': pl.verts, 'joints_right': pr.joints, 'joints_conf_right': pr.joints_conf, 'init_left': pl.init, 'init_right': pr.init}
    np.savez(str(tmp_path / 'T.npz'), **tg)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    common = ['--model', ck, '--targets', str(tmp_path / 'T.npz'), '--iters', '20', '--lr', '0.1', '--center', str(R.CENTER), '--bs', '3']
    out = {}
    for name, extra in (('closed', ['--start', 'closed']), ('neutral', ['--start', 'neutral']), ('plain', [])):
        assert A.main(common + ['--out', str(tmp_path / (name + '.npz'))] + extra) == 8
        with np.load(str(tmp_path / (name + '.npz'))) as f:
            out[name] = {k: f[k] for k in f.files}
    assert sorted(out['plain']) == sorted(out['neutral']) and all(np.array_equal(out['plain'][k], out['neutral'][k], equal_nan=True) for k in out['plain'])
    new = sorted('%s_%s' % (k, s) for s in ('left', 'right') for k in ('start', 'start_status', 'start_choice'))
    assert sorted(set(out['closed']) - set(out['plain'])) == new and set(out['plain']) <= set(out['closed'])
    tabs, keep = A.tables_from_checkpoint(state, R.CENTER)
    w = {'w_verts': 1e4, 'w_joints': 1e4, 'w_uv': 0.0}
    lib = MF.fit_mano([tabs['left'], tabs['right']], [dev(pl.init), dev(pr.init)], verts=[dev(pl.verts), None], joints=[None, dev(pr.joints)],
                      joints_conf=[None, dev(pr.joints_conf)], iters=20, lr=0.1, weights=w, start='closed')
    st = MF.start_mano([tabs['left'], tabs['right']], [dev(pl.init), dev(pr.init)], verts=[dev(pl.verts), None], joints=[None, dev(pr.joints)],
                       joints_conf=[None, dev(pr.joints_conf)], weights=w)
    for h, s in enumerate(('left', 'right')):
        assert np.array_equal(out['closed']['para_' + s], lib.para[h].cpu().numpy()) and np.array_equal(out['closed']['start_' + s], st.para[h].cpu().numpy())
        assert out['closed']['start_status_' + s].tolist() == [0] * 4 and out['closed']['start_choice_' + s].tolist() == [-1] * 4
        assert out['closed']['start_status_' + s].dtype == np.int32 and not np.array_equal(out['closed']['para_' + s], out['plain']['para_' + s])
        k = 0 if s == 'left' else 1
        print(s, 'RMS mm after 20 iterations: neutral', (np.sqrt(out['plain']['mse_after_' + s][:, k]) * 1e3).tolist(), 'closed', (np.sqrt(out['closed']['mse_after_' + s][:, k]) * 1e3).tolist())
