"""CPU: the float64 restatement of dir_mano_fit_start's rule (tests/helpers/mano_start_ref.py) has the properties the rule is there for -- it recovers
a rigid rotation of the targets, is equivariant, never worsens the terms it looks at, uses only the points that are rigid under the root, picks the
right one of the cube's rotations from 2-D targets with a camera of positive scale -- and it buys the fit what the feature is for (the value test).
The recorded float32-against-float64 differences (GATES) that bound the GPU test are re-measured here."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import mano_cases as M  # noqa: E402
import mano_fit_ref as R  # noqa: E402
import mano_start_ref as S  # noqa: E402

F64 = torch.float64


def forward64(p, side, center=R.CENTER, root_palm=False, root_mat=None):
    with torch.no_grad():
        v, j, u, _ = M.mano_outputs(S.KIND, side, center, torch.as_tensor(np.asarray(p), dtype=F64), root_palm, root_mat=root_mat, fold=True)
    return v.numpy(), j.numpy(), u.numpy()


def problem(side, init, verts=None, joints=None, jconf=None, uv=None, uconf=None, center=R.CENTER, root_palm=False, w_verts=1e4, w_joints=1e4):
    w = dict(dict.fromkeys(R.WEIGHTS, 0.0), w_verts=w_verts if verts is not None else 0.0, w_joints=w_joints if joints is not None else 0.0, w_uv=1.0 if uv is not None else 0.0)
    return R.Problem('t_' + side, side, center, root_palm, init, verts, joints, jconf, uv, uconf, w, (0.1,) * 4)


@pytest.mark.parametrize('side', ['right', 'left'])
def test_recovery_of_a_rigid_rotation(side):
    """targets = the forward at (Q* R0, the same PCA, betas, camera): the root written is Q* R0 to 1e-9 rad, from joints, from vertices and from both;
    with Q* = I the root may be rewritten with R0's columns"""
    p0 = R.truth(4, side).astype(np.float64)
    R0 = S.root_of(p0)
    r = M._rng('start.recovery.' + side)
    for center, root_palm in ((R.CENTER, False), (0, False), (-1, False), (R.CENTER, True)):
        Qs = torch.from_numpy(np.stack([S.rotation(r.normal(0, 1, 3), a) for a in (0.5, 2.0, np.pi - 1e-3, 0.0)]))
        v, j, _ = forward64(p0, side, center, root_palm, root_mat=Qs @ R0)
        for kind in ('joints', 'verts', 'both'):
            prob = problem(side, p0, v if kind != 'joints' else None, j if kind != 'verts' else None, center=center, root_palm=root_palm)
            res = S.start(prob, F64)
            ang = S.angle_between(res['R1'], Qs @ R0)
            ang_p = S.angle_between(S.root_of(res['para']), Qs @ R0)
            print(side, center, root_palm, kind, 'angle to Q* R0', ang.tolist(), 'status', res['status'].tolist(), 'e1', res['info'][:, 1].tolist())
            assert res['status'].tolist()[:3] == [0] * 3 and res['status'].tolist()[3] in (0, 8)      # Q* = I: e0 is exactly 0, the root may stay
            assert float(ang.max()) <= 1e-9 and float(ang_p.max()) <= 1e-9
            assert torch.equal(res['para'][:, 6:], torch.from_numpy(p0)[:, 6:])


def test_equivariance():
    """rotating the targets by G about the pivot gives G R1, to 1e-9 rad"""
    for side in ('right', 'left'):
        prob, _ = S.case('mesh', side)
        jprob, _ = S.case('joints', side)
        prob = prob._replace(joints=jprob.joints, joints_conf=jprob.joints_conf, weights=dict(prob.weights, w_joints=1e4))
        base = S.start(prob, F64)
        G = S.rotation([0.3, -1.0, 0.5], 1.7)
        rot = lambda a: None if a is None else np.asarray(a, np.float64) @ G.T  # noqa: E731      (centre 9: the pivot is 0)
        got = S.start(prob._replace(verts=rot(prob.verts), joints=rot(prob.joints)), F64)
        ang = S.angle_between(got['R1'], torch.from_numpy(G) @ base['R1'])
        print(side, 'equivariance angle', ang.tolist())
        assert base['status'].tolist() == got['status'].tolist() == [0, 0, 0] and float(ang.max()) <= 1e-9
        assert float((got['info'][:, 1] - base['info'][:, 1]).abs().max()) <= 1e-9 * float(base['info'][:, 1].max())


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_never_worse(name):
    """random articulated hands whose betas differ from the start's: e1 <= e0 and the 2-D residual after <= before on every row -- by `info`, and by the
    forward at the started parameters itself"""
    for side in ('right', 'left'):
        prob, _ = S.case(name, side, 4)
        res = S.start(prob, F64)
        info = res['info']
        print(name, side, 'info', info.tolist(), 'status', res['status'].tolist())
        assert res['status'].tolist() == [0] * 4
        assert bool((info[:, 1] <= info[:, 0]).all()) and bool((info[:, 3] <= info[:, 2]).all())
        if name != 'mesh' and name != 'joints':
            assert bool((info[:, 3] < 0.5 * info[:, 2]).all())                 # the camera is fitted, not merely kept
        # the energies from the forward at p_out: left-multiplying the root is what the closed form says it is
        v, j, u = forward64(res['para'].numpy(), side, prob.center, prob.root_palm)
        if prob.joint_uv is not None:
            d = np.where(prob.uv_conf > 0, prob.uv_conf, 0.0)
            e = (d * (np.where(d[..., None] > 0, u - prob.joint_uv.astype(np.float64), 0.0) ** 2).sum(-1)).sum(1)
            assert np.abs(e - info[:, 3].numpy()).max() <= 1e-6 * info[:, 3].numpy().max() and (e <= info[:, 2].numpy()).all()
        e3 = np.zeros(4)
        if prob.verts is not None:
            w = float(np.float32(prob.weights['w_verts'] / 778.0)) * M._tt(S.KIND, side, F64)['weights'][:, 0].numpy()
            e3 += (w * ((v - prob.verts.astype(np.float64)) ** 2).sum(-1)).sum(1)
        if prob.joints is not None:
            rs = [k for k in S.RS if not (k == 0 and prob.root_palm)]
            c = np.where(prob.joints_conf > 0, prob.joints_conf, 0.0)[:, rs].astype(np.float64) * float(np.float32(prob.weights['w_joints'] / 21.0))
            e3 += (c * (np.where(c[..., None] > 0, j[:, rs] - prob.joints[:, rs].astype(np.float64), 0.0) ** 2).sum(-1)).sum(1)
        if prob.verts is not None or prob.joints is not None:
            assert np.abs(e3 - info[:, 1].numpy()).max() <= 1e-6 * info[:, 1].numpy().max() and (e3 <= info[:, 0].numpy()).all()


def test_only_rigid_joints_count():
    """joints as the only target: changing the target's non-RS joints leaves p_out bit for bit (and with root_palm joint 0 is one of those)"""
    for root_palm in (False, True):
        prob, _ = S.case('joints', 'right')
        prob = prob._replace(root_palm=root_palm)
        base = S.start(prob, F64)
        moved = prob.joints.copy()
        rs = [k for k in S.RS if not (k == 0 and root_palm)]
        others = [k for k in range(21) if k not in rs and k != 11 and k != 5]
        moved[:, others] += np.float32(0.05)
        got = S.start(prob._replace(joints=moved), F64)
        assert torch.equal(base['para'], got['para']) and base['status'].tolist() == [0, 0, 0]
        touched = prob.joints.copy()
        touched[:, 13] += np.float32(0.05)                 # (joint 9 is the centre: its model point is the pivot itself)
        assert not torch.equal(base['para'], S.start(prob._replace(joints=touched), F64)['para'])


def test_selection_and_degeneracy():
    prob, _ = S.case('joints', 'left')
    base = S.start(prob, F64)
    p0 = torch.from_numpy(prob.init).double()
    # a rigid joint at confidence 0 holding NaN is selected out: the same as finite garbage there
    junk = prob.joints.copy()
    junk[np.isnan(junk)] = 12345.0
    assert np.isnan(prob.joints[:, 5]).all() and base['status'].tolist() == [0, 0, 0] and torch.equal(base['para'], S.start(prob._replace(joints=junk), F64)['para'])
    # NaN under a confidence > 0: the row passes through
    conf = prob.joints_conf.copy()
    conf[1, 11] = 0.5
    r = S.start(prob._replace(joints_conf=conf), F64)
    assert r['status'].tolist() == [0, 2, 0] and torch.equal(r['para'][1], p0[1]) and torch.equal(r['para'][0], base['para'][0])
    # every rigid joint dropped, no vertices: status 8, p0's root
    conf = prob.joints_conf.copy()
    conf[:, list(S.RS)] = 0.0
    r = S.start(prob._replace(joints_conf=conf), F64)
    assert r['status'].tolist() == [8, 8, 8] and torch.equal(r['para'], p0)
    # two selected keypoints at one position: no scale to fit -> status 16, p0's camera (the root still comes from the joints)
    uprob, _ = S.case('root_palm', 'left')
    uconf = np.zeros_like(uprob.uv_conf)
    uconf[:, [3, 7]] = 1.0
    uv = uprob.joint_uv.copy()
    uv[:, 7] = uv[:, 3]
    r = S.start(uprob._replace(joint_uv=uv, uv_conf=uconf), F64)
    assert r['status'].tolist() == [16, 16, 16] and torch.equal(r['para'][:, 61:64], torch.from_numpy(uprob.init).double()[:, 61:64])
    assert not torch.equal(r['para'][:, :6], torch.from_numpy(uprob.init).double()[:, :6])
    # the switches leave their groups
    aprob, _ = S.case('all', 'right')
    full = S.start(aprob, F64)
    a0 = torch.from_numpy(aprob.init).double()
    nr, nc = S.start(aprob, F64, root=False), S.start(aprob, F64, cam=False)
    assert torch.equal(nr['para'][:, :6], a0[:, :6]) and not torch.equal(nr['para'][:, 61:], a0[:, 61:])
    assert torch.equal(nc['para'][:, 61:], a0[:, 61:]) and torch.equal(nc['para'][:, :6], full['para'][:, :6])
    sprob, _ = S.case('uv', 'right')
    ns = S.start(sprob, F64, search=False)
    s0 = torch.from_numpy(sprob.init).double()
    assert torch.equal(ns['para'][:, :6], s0[:, :6]) and ns['choice'].tolist() == [-1] * 3 and not torch.equal(ns['para'][:, 61:], s0[:, 61:])


def test_the_candidates():
    P = S.cube_rotations()
    assert P.shape == (24, 3, 3) and np.array_equal(P[0], np.eye(3, dtype=np.int64))
    assert len({p.tobytes() for p in P}) == 24 and all(round(np.linalg.det(p)) == 1 for p in P)
    have = {p.tobytes() for p in P}
    assert all((a @ b).tobytes() in have for a in P for b in P)
    assert all(np.abs(p).sum(0).tolist() == [1, 1, 1] and np.abs(p).sum(1).tolist() == [1, 1, 1] for p in P)


def search_problem(side):
    """24 articulated hands; row k's 2-D targets are the forward at root P_k R0 under a camera of its own (s in [2.5, 5], float64 targets)"""
    p0 = R.truth(24, side, seed=1).astype(np.float64)
    r = M._rng('start.search.' + side)
    cam = np.stack([r.uniform(2.5, 5.0, 24), r.normal(0, 0.1, 24), r.normal(0, 0.1, 24)], 1)
    q = p0.copy()
    q[:, 61:64] = cam
    Ps = torch.from_numpy(S.cube_rotations()).double()
    _, _, u = forward64(q, side, root_mat=Ps @ S.root_of(p0))
    return problem(side, p0, uv=u, uconf=np.ones((24, 21))), cam


TIPS = (4, 8, 12, 16, 20)


@pytest.mark.parametrize('side', ['right', 'left'])
def test_search_recovers_a_candidate(side):
    """row k's targets come from root P_k R0: choice == k on every row, and the camera comes back to 1e-9 from the 16 keypoints that are chain joints.
    The five fingertips are skinned vertices, for which "left-multiplying the root rotates the output about the pivot" holds to 6e-10 m only (a float32
    skinning row does not sum to 1, include/dir_hip.h step 1): with all 21 keypoints the scale can be off by s x 6e-10 m / the keypoints' spread
    (>= 0.03 m) = 5 x 2e-8 = 1e-7, which is the bound there (measured: 6.8e-9 right, 9.3e-9 left)."""
    prob, cam = search_problem(side)
    chain = np.ones((24, 21))
    chain[:, TIPS] = 0.0
    Ps = torch.from_numpy(S.cube_rotations()).double()
    for conf, bound in ((chain, 1e-9), (np.ones((24, 21)), 1e-7)):
        res = S.start(prob._replace(uv_conf=conf), F64)
        err = (res['para'][:, 61:64] - torch.from_numpy(cam)).abs().max()
        print(side, int(conf.sum(1)[0]), 'keypoints: choice', res['choice'].tolist(), 'camera error %.3g' % float(err), 'residual', res['info'][:, 3].max().item())
        assert res['choice'].tolist() == list(range(24)) and res['status'].tolist() == [0] * 24
        assert float(err) <= bound and bool((res['para'][:, 61] > 0).all())
        assert float(S.angle_between(S.root_of(res['para']), Ps @ S.root_of(prob.init)).max()) <= 1e-9
    # mirrored targets (u -> -u): the least-squares scale of the best-fitting candidate would be negative; no selected camera has s <= 0
    mir = S.start(prob._replace(joint_uv=-np.asarray(prob.joint_uv)), F64)
    assert bool((mir['para'][:, 61] > 0).all())


def uv_problems():
    """every 2-D-only problem a test uses (rows are prefix-stable in n: 5 covers the GPU tests' and the value test's rows)"""
    return [S.case('uv', side, 5)[0] for side in ('right', 'left')]


def test_search_gap():
    """the float64 gap between the best and the second-best e_k is at least 1e-3 of the best: a float32 run cannot pick another candidate"""
    for prob in uv_problems():
        e = S.start(prob, F64)['e_k'].sort(1).values
        gap = (e[:, 1] - e[:, 0]) / e[:, 0]
        print(prob.name, 'gap / best', gap.tolist())
        assert bool((gap >= 1e-3).all())
        assert S.start(prob, torch.float32)['choice'].tolist() == S.start(prob, F64)['choice'].tolist()
    for a, b in ((3, 5), (4, 5)):
        assert np.array_equal(S.case('uv', 'left', a)[0].joint_uv, S.case('uv', 'left', b)[0].joint_uv[:a])


VALUE_CASES = (('mesh', 'right', (50, 200)), ('joints', 'left', (50, 200)), ('uv', 'left', (400,)))


@pytest.mark.parametrize('name,side,iters', VALUE_CASES)
def test_value_of_the_start(name, side, iters):
    """the far-rotation cases, 4 rows: mano_fit_ref.fit from the cold start and from the restated start; the started fit ends below the cold fit on every
    row -- the term's RMS at 50 and at 200 iterations (mesh, joints), the root's angle to the truth at 400 (2-D)"""
    prob, truth = S.case(name, side, 4)
    started = S.start(prob, F64)['para'].numpy()
    term = {'mesh': 0, 'joints': 1, 'uv': 2}[name]
    fig = {}
    for label, init in (('cold', np.asarray(prob.init, np.float64)), ('started', started)):
        res, done, state = None, 0, None
        for it in iters:
            res = R.fit(prob, it - done, F64, state=state, anchor=init, init=init if res is None else res['para'].numpy())
            state, done = res['state'], it
            if name == 'uv':
                fig[(label, it)] = S.angle_between(S.root_of(res['para']), S.root_of(truth)).numpy()
            else:
                fig[(label, it)] = res['mse_after'][:, term].sqrt().numpy() * 1e3
    for it in iters:
        cold, st = fig[('cold', it)], fig[('started', it)]
        print(name, side, it, 'iterations: cold', np.round(cold, 5).tolist(), 'started', np.round(st, 5).tolist(), 'ratio', np.round(cold / st, 2).tolist(),
              'mm RMS' if name != 'uv' else 'rad to the truth')
        assert (st < cold).all(), (name, it, cold, st)
        lo, hi = S.VALUE[name][it]
        assert lo[0] * 0.5 <= cold.min() and cold.max() <= hi[0] * 2.0 and st.max() <= hi[1] * 2.0, 'the record in mano_start_ref.VALUE is stale'


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_gates_are_what_the_restatement_measures(name):
    got = S.measure(name)
    for k in S.OUTPUTS:
        print(name, k, 'measured %.3g recorded %.3g' % (got[k], S.GATES[name][k]))
    for k in S.OUTPUTS:
        assert got[k] <= S.GATES[name][k], (name, k, got[k], S.GATES[name][k])
