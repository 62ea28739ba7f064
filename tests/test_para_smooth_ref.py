"""CPU only: the float64 restatement of dir_mano_para_smooth_step's rule (tests/helpers/para_smooth_ref.py) against things already pinned
(mano_cases.mano_outputs, OneEuroRef) and against closed forms; the GATES the GPU test uses are re-measured here; pose_aa_to_pca; and the
entry point's host side (state layout, argument errors before any launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import mano_cases as M  # noqa: E402
import para_smooth_ref as P  # noqa: E402
from one_euro_ref import OneEuroRef  # noqa: E402

F64 = torch.float64


def six_of(R):
    return np.concatenate([R[:, 0], R[:, 1]])


def para_of(R, pca=None, betas=None):
    p = np.zeros(64, np.float64)
    p[:6] = six_of(R)
    if pca is not None:
        p[6:51] = pca
    if betas is not None:
        p[51:61] = betas
    return p


def step64(ref, paras, cam=None, valid=None):
    """ref.step on float64 rows WITHOUT the float32 rounding of the inputs (closed forms hold to 1e-12 only then)"""
    para = torch.as_tensor(np.asarray(paras, np.float64).reshape(-1, 64))
    cam = torch.tensor([[200.0, 300.0, 250.0]], dtype=F64).repeat(para.shape[0], 1) if cam is None else torch.as_tensor(np.asarray(cam, np.float64))
    return ref.step(para, cam, valid)


def log_angle(R, axis):
    """the rotation angle of R [3,3] about the unit `axis`"""
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(s @ axis, 0.5 * (np.trace(R) - 1.0)))


def test_forward_equals_the_pinned_restatement():
    for side in ('left', 'right'):
        for root_palm in (False, True):
            p = torch.from_numpy(P.parity_case(side)[0]['para'].astype(np.float64))
            R = M.robust_rot6d(p[:, :6])
            v, j, _, _ = M.mano_outputs(P.KIND, side, P.CENTER, p, root_palm, root_mat=R, fold=True)
            v2, j2 = P.forward(side, P.CENTER, root_palm, R, P.pose_aa(side, p[:, 6:51]), p[:, 51:61])
            assert float((v - v2).abs().max()) <= 1e-12 and float((j - j2).abs().max()) <= 1e-12


def test_finger_and_camera_streams_are_the_one_euro_rule():
    """shape_frames = 0, the case's valid flags and gap: smoothed[6:51] and [61:64] equal OneEuroRef on the same numbers.  pd_offset never enters
    this rule: ParameterSmoother sends it through OneEuro itself, which tests/test_smooth_ref.py pins."""
    side = 'right'
    frames = P.parity_case(side)
    outs, ref = P.run_case(side, F64, frames, shape_frames=0)
    oe = OneEuroRef([(15, 3, 100.0), (3, 1, 1.0)], P.SEQS, fps=30.0, max_gap=4)
    for f, o in zip(frames, outs):
        aa = P.pose_aa(side, torch.from_numpy(f['para'][:, 6:51].astype(np.float64))).numpy()
        y, upd = oe.step(np.concatenate([aa, f['cam_px'].astype(np.float64)], 1), f['valid'])
        assert (upd == o['updated']).all()
        got = torch.cat([o['smoothed'][:, 6:51], o['smoothed'][:, 61:64]], 1).numpy()
        assert np.abs(got - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    assert (ref.age == oe.age).all() and (ref.run == oe.run).all() and (ref.count == oe.count).all()


def test_constant_input_returns_itself():
    side = 'left'
    f = P.parity_case(side)[0]
    ref = P.ParaSmoothRef(side, P.SEQS, dt=F64, **P.CASE_OPTS)
    first = None
    for t in range(6):
        o = ref.step(f['para'], f['cam_px'])
        first = o if first is None else first
        for k in ('smoothed', 'verts', 'joints', 'joints_px'):      # the input six is not normalised: the ROTATION returns itself, below
            a, b = (o[k], first[k]) if k != 'smoothed' else (o[k][:, 6:], first[k][:, 6:])
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (t, k)
        Rx = M.robust_rot6d(torch.from_numpy(f['para'][:, :6].astype(np.float64)))
        assert float((M.robust_rot6d(o['smoothed'][:, :6]) - Rx).abs().max()) <= 1e-12
    assert ref.measures[:, [1, 3, 5, 7]].max() <= 1e-9 and (ref.count == 4).all()


def test_root_step_response_is_the_scalar_filter_of_the_angle():
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    base = P._rot(np.array([1.0, 2.0, -1.0]), 0.7)
    ref = P.ParaSmoothRef('right', 1, dt=F64, fps=30.0, beta=0.0, max_gap=4, shape_frames=0)
    oe = OneEuroRef([(1, 1, 1.0)], 1, fps=30.0, beta=0.0, max_gap=4)
    for t in range(10):
        ang = 0.2 * t
        o = step64(ref, para_of(base @ P._rot(axis, ang)))
        y, _ = oe.step(np.array([[ang]]))
        Ry = M.robust_rot6d(o['smoothed'][:, :6])[0].numpy()
        assert abs(log_angle(base.T @ Ry, axis) - y[0, 0]) <= 1e-12, t


def test_equivariance_about_the_wrist():
    side = 'left'
    frames = P.parity_case(side)
    Q = P._rot(np.array([0.2, 0.9, -0.4]), 1.1)
    Qt = torch.from_numpy(Q)
    a = P.ParaSmoothRef(side, P.SEQS, dt=F64, center=0, **P.CASE_OPTS)
    b = P.ParaSmoothRef(side, P.SEQS, dt=F64, center=0, **P.CASE_OPTS)
    for f in frames[:6]:
        pa = torch.from_numpy(f['para'].astype(np.float64))
        pa[torch.isnan(pa)] = 0.0
        pb = pa.clone()
        pb[:, 0:3], pb[:, 3:6] = pa[:, 0:3] @ Qt.t(), pa[:, 3:6] @ Qt.t()
        cam = torch.from_numpy(f['cam_px'].astype(np.float64))
        oa, ob = a.step(pa, cam, f["valid"]), b.step(pb, cam, f["valid"])
        assert (oa['updated'] == ob['updated']).all()
        # the rule itself: the filtered rotation turns with Q, every other parameter stays
        assert float((M.robust_rot6d(ob['smoothed'][:, :6]) - Qt @ M.robust_rot6d(oa['smoothed'][:, :6])).abs().max()) <= 1e-12
        assert float((ob['smoothed'][:, 6:] - oa['smoothed'][:, 6:]).abs().max()) <= 1e-12
        # the forward: vertex v is (sum_k w_vk) J_0 + R_0 (...) before centring, and the float32 skinning weights of a vertex do not sum to 1
        # exactly: the part (sum_k w_vk - 1) J_0 does not turn.  The bound is that part (for both runs) plus the 1e-12 of the other checks
        T = M._tt(P.KIND, side, F64)
        j0 = (T['j_template'][0] + torch.einsum('ck,bk->bc', T['j_shapedirs'][0], oa['smoothed'][:, 51:61])).norm(dim=1).max()
        tol = 2.0 * float((T['weights'].sum(1) - 1.0).abs().max() * j0) + 1e-12
        assert tol < 1e-8
        for k in ('verts', 'joints'):
            assert float((ob[k] - oa[k] @ Qt.t()).abs().max()) <= tol, k
        chain = [j for j in range(21) if j % 4 != 0 or j == 0]          # chain joints carry no skinning weight: they turn exactly
        assert float((ob['joints'][:, chain] - oa['joints'][:, chain] @ Qt.t()).abs().max()) <= 1e-12


def test_shape_is_a_running_mean_then_frozen_and_bones_keep_their_length():
    side = 'right'
    frames = P.parity_case(side)
    allv = [dict(f, valid=np.ones(P.SEQS, np.int32)) for f in frames]
    outs, ref = P.run_case(side, F64, allv, shape_frames=3)
    b = np.stack([f['para'][:, 51:61].astype(np.float64) for f in frames])
    for t, o in enumerate(outs):
        want = b[:min(t + 1, 3)].mean(0)
        assert np.abs(o['smoothed'][:, 51:61].numpy() - want).max() <= 1e-12, t
    assert (ref.n_shape == 3).all()
    L = torch.stack([P.bone_lengths(o['joints'], P.RIGID) for o in outs[2:]])
    assert float((L - L[0]).abs().max()) <= 1e-12                    # the 15 rigid bones: constant from the freeze on
    tips = torch.stack([P.bone_lengths(o['joints'], [x for x in P.BONES if x not in P.RIGID]) for o in outs[2:]])
    assert float((tips - tips[0]).abs().max()) > 1e-6                # tip bones end in skinned vertices: not rigid
    outs0, _ = P.run_case(side, F64, allv, shape_frames=0)
    L0 = torch.stack([P.bone_lengths(o['joints'], P.RIGID) for o in outs0[2:]])
    assert float((L0 - L0[0]).abs().max()) > 1e-5                    # without a fixed shape the lengths follow the betas


def test_a_gap_reinitialises_the_pose_and_keeps_the_shape():
    side = 'right'
    frames = P.parity_case(side)
    outs, ref = P.run_case(side, F64, frames)
    upd = np.stack([o['updated'] for o in outs])
    assert upd[:, 1].tolist() == [2, 1, 1, 0, 0, 0, 0, 0, 2, 1, 1, 1] and upd[:, 0].tolist() == [2, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    frozen = outs[2]['smoothed'][1, 51:61]
    for t in (8, 9, 11):
        assert torch.equal(outs[t]['smoothed'][1, 51:61], frozen)
    x8 = torch.from_numpy(frames[8]['para'][1].astype(np.float64))
    assert torch.equal(outs[8]['smoothed'][1, :6], x8[:6])           # re-initialised: the pose is the input's
    # a passed-through row is the forward at its own parameters
    p = torch.from_numpy(frames[3]['para'].astype(np.float64))
    v, j = P.forward(side, P.CENTER, False, M.robust_rot6d(p[:, :6]), P.pose_aa(side, p[:, 6:51]), p[:, 51:61])
    assert torch.equal(outs[3]['verts'][0], v[0]) and torch.equal(outs[3]['joints'][1], j[1])


def test_case_stays_inside_the_log_maps_good_range():
    for side in ('left', 'right'):
        frames = P.parity_case(side)
        for q in range(P.SEQS):
            Rs = [M.robust_rot6d(torch.from_numpy(f['para'][q:q + 1, :6].astype(np.float64)))[0].numpy() for f in frames]
            for a, b in zip(Rs, Rs[1:]):
                assert np.arccos(np.clip(0.5 * (np.trace(a.T @ b) - 1.0), -1, 1)) <= 0.5
        p = torch.from_numpy(np.nan_to_num(np.concatenate([f['para'] for f in frames]).astype(np.float64)))
        assert float(P.pose_aa(side, p[:, 6:51]).reshape(-1, 15, 3).norm(dim=-1).max()) < 2.0


def test_relative_rotation_near_pi_breaks_and_tiny_ones_are_finite():
    base = P._rot(np.array([0.1, 0.7, -0.3]), 0.4)
    axis = np.array([0.0, 0.6, 0.8])
    for dt in (F64, torch.float32):
        ref = P.ParaSmoothRef('right', 1, dt=dt, fps=30.0, max_gap=4, shape_frames=0)
        assert ref.step(para_of(base)[None], [[200.0, 300.0, 250.0]])['updated'].tolist() == [2]
        o = ref.step(para_of(base @ P._rot(axis, np.pi))[None], [[200.0, 300.0, 250.0]])
        assert o['updated'].tolist() == [2] and ref.run[0] == 1      # exactly pi: n = 0 (to rounding), c = -1: a break
        for ang in (0.0, 1e-7):
            ref = P.ParaSmoothRef('right', 1, dt=dt, fps=30.0, max_gap=4, shape_frames=0)
            ref.step(para_of(base)[None], [[200.0, 300.0, 250.0]])
            o = ref.step(para_of(base @ P._rot(axis, ang))[None], [[200.0, 300.0, 250.0]])
            R = M.robust_rot6d(o['smoothed'][:, :6])[0].double()
            assert o['updated'].tolist() == [1] and bool(torch.isfinite(o['verts']).all())
            assert float((R.t() @ R - torch.eye(3, dtype=F64)).abs().max()) <= (1e-12 if dt == F64 else 1e-6)


def test_pose_aa_to_pca_round_trips():
    from dir_amd.utils.smooth import pose_aa_to_pca
    for side in ('left', 'right'):
        buf = M.tables(P.KIND, side)
        pca = torch.from_numpy(M._rng('aa2pca').normal(0, 0.5, (4, 45)))
        aa = P.pose_aa(side, pca)
        back = pose_aa_to_pca({'th_selected_comps': buf['th_selected_comps'], 'th_hands_mean': buf['th_hands_mean']}, aa)
        assert float((back - pca).abs().max()) <= 1e-10
        with pytest.raises(ValueError):
            pose_aa_to_pca((buf['th_selected_comps'][:30], buf['th_hands_mean']), aa)
        sing = buf['th_selected_comps'].copy()
        sing[7] = sing[3]
        with pytest.raises(ValueError):
            pose_aa_to_pca((sing, buf['th_hands_mean']), aa)


def test_gates_are_re_measured():
    """GATES: the largest |float32 run - float64 run| of the restatement per output over the canonical case; a re-measured figure above its
    record fails"""
    got = P.measure()
    print('re-measured', got)
    assert set(got) == set(P.GATES) == set(P.OUTPUTS)
    for k, v in got.items():
        assert v <= P.GATES[k], (k, v, P.GATES[k])
        assert v >= P.GATES[k] / 50.0, (k, v, P.GATES[k])            # a record far above what is measured gates nothing


def test_state_layout_and_argument_errors_before_any_launch():
    from dir_amd import _capi
    L = _capi.lib()
    off = (ctypes.c_longlong * len(_capi.MANO_PARA_SMOOTH_FIELDS))()
    row = L.dir_mano_para_smooth_state_bytes(off)
    o = dict(zip(_capi.MANO_PARA_SMOOTH_FIELDS, off))
    assert row == L.dir_mano_para_smooth_state_bytes(None) and row % 16 == 0
    assert o['measures'] == 0 and o['y1'] % 16 == 0 and o['y2'] - o['y1'] == o['x1'] - o['y2'] == o['x2'] - o['x1'] == o['prev'] - o['x2'] == 2440 * 4
    assert o['vel'] - o['prev'] == 256 and o['n_shape'] - o['vel'] == 256 and [o[k] - o['n_shape'] for k in ('age', 'run', 'count')] == [4, 8, 12]
    assert row == o['count'] + 4

    one = 4096
    T = _capi.ManoTables(one, one, one, one, one, one, one, one, 0, 9, 0)
    H = _capi.ManoParaSmoothHand(*([one] * 11))
    good = dict(fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, rot_speed_scale=100.0, cam_speed_scale=1.0, max_gap=4, shape_frames=3)

    def bad(word, tables=T, hand=H, hands=1, B=1, **kw):
        opts = _capi.ManoParaSmoothOpts(**dict(good, **kw))
        rc = L.dir_mano_para_smooth_step(tables, hand, None, ctypes.byref(opts), hands, B, None)
        assert rc == -1 and word in L.dir_last_error(), (rc, L.dir_last_error())
    bad(b'null pointer', tables=None)
    bad(b'null pointer', hand=None)
    bad(b'null pointer', hand=_capi.ManoParaSmoothHand(*([one] * 10 + [None])))
    bad(b'null pointer', hand=_capi.ManoParaSmoothHand(*([None] + [one] * 10)))
    bad(b'B 0 outside', B=0)
    bad(b'outside', B=4097)
    bad(b'hands 3', hands=3)
    bad(b'hands 0', hands=0)
    for kw in (dict(fps=0.0), dict(min_cutoff=-1.0), dict(d_cutoff=0.0), dict(beta=-0.1), dict(max_gap=0), dict(shape_frames=-1), dict(fps=float('nan'))):
        bad(b'non-positive rate', **kw)
    rc = L.dir_mano_para_smooth_step(T, H, None, None, 1, 1, None)
    assert rc == -1 and b'null pointer' in L.dir_last_error()
