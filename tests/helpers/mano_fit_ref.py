"""TEST INFRASTRUCTURE (CPU only: torch CPU): the rule of dir_mano_fit (include/dir_hip.h, "MANO fitting") restated in torch, parametrised by
dtype.  The forward is mano_cases.mano_outputs (pinned to the reference through oracle/mano.py) in the kernels' order (fold=True); the gradient is
autograd through it in the run's dtype (float64: the reference) for the cotangents the header names; the priors' gradients and Adam are written
out by hand, operation for operation as the header orders them.

CANONICAL CASES   tables synth.mano_buffers (table set 'pca'), centre 9, `truth(n, side)` = n random hands (0.16 .. 0.22 m across):
    'mesh'     cold start (neutral_para, cam scale 4), vertex term only (w_verts 1e4), lr 0.03 on every group
    'joints'   cold start, 3-D joints with confidences in (0.2, 1] and two joints per hand at confidence 0 whose targets hold NaN (w_joints 1e4), lr 0.03
    'uv'       refinement: truth + noise (0.05 on the 6D root, 0.15 on PCA, 0.03 on cam), 2-D term only (w_uv 1), w_init 1e-3, betas frozen, lr 0.01,
               one keypoint per hand at confidence 0 holding NaN

GATES   GATES[config][iters] = the largest |restatement float32 - restatement float64| per output over truth(3, side), both sides, recorded here
from a CPU run and re-measured by tests/test_mano_fit_ref.py (which fails when a re-measured figure exceeds its record).  The GPU test allows
MARGIN = 4 x the record (the project's margin for another valid summation order).  Nothing here is measured on the kernel.
"""
import collections
import os
import sys

import numpy as np
import torch

_here = os.path.dirname(os.path.abspath(__file__))
if _here not in sys.path:
    sys.path.insert(0, _here)
import mano_cases as M  # noqa: E402

KIND, CENTER = 'pca', 9
GROUP_SLICES = (slice(0, 6), slice(6, 51), slice(51, 61), slice(61, 64))
WEIGHTS = ('w_verts', 'w_joints', 'w_uv', 'w_pca', 'w_beta', 'w_init')
MARGIN = 4.0
ITERS = (1, 2, 10, 50)
OUTPUTS = ('para', 'verts', 'joints', 'joint_uv', 'mse_after')


def neutral_para(n, cam_scale=1.0, dt=torch.float64):
    p = torch.zeros(n, 64, dtype=dt)
    p[:, 0] = 1.0
    p[:, 4] = 1.0
    p[:, 61] = cam_scale
    return p


def truth(n, side, seed=0):
    """n random hands as float32 parameters [n,64] (numpy): the root a rotation by up to 1 rad about a random axis, its first two columns scaled
    by 0.7 .. 1.4 (the 6D input is not normalised), PCA coefficients N(0, 0.4), betas N(0, 0.5), cam scale in [3.5, 4.5], translations N(0, 0.1).
    (A cold start from the identity root does not reach an arbitrary rotation in a few hundred steps; this range is what 200 steps at lr 0.1 fit to
    micrometres in float64, tests/test_mano_fit_ref.py.)"""
    r = M._rng('fit.truth.%s.%d' % (side, seed))
    out = np.zeros((n, 64), np.float32)
    for i in range(n):
        ax = r.normal(0, 1, 3)
        ax /= np.linalg.norm(ax)
        ang = r.uniform(0.0, 1.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        rot = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        out[i, 0:3], out[i, 3:6] = rot[:, 0] * r.uniform(0.7, 1.4), rot[:, 1] * r.uniform(0.7, 1.4)
        out[i, 6:51] = r.normal(0, 0.4, 45)
        out[i, 51:61] = r.normal(0, 0.5, 10)
        out[i, 61] = r.uniform(3.5, 4.5)
        out[i, 62:64] = r.normal(0, 0.1, 2)
    return out


def targets_of(para, side, center=CENTER, root_palm=False):
    """float32 targets of float32 parameters: the float64 forward rounded once -> dict verts [n,778,3], joints [n,21,3], joint_uv [n,21,2] (numpy)"""
    with torch.no_grad():
        v, j, u, _ = M.mano_outputs(KIND, side, center, torch.from_numpy(para.astype(np.float64)), root_palm, fold=True)
    return {'verts': v.numpy().astype(np.float32), 'joints': j.numpy().astype(np.float32), 'joint_uv': u.numpy().astype(np.float32)}


Problem = collections.namedtuple('Problem', 'name side center root_palm init verts joints joints_conf joint_uv uv_conf weights lr')


def problem(config, n, side, seed=0, root_palm=False):
    """the canonical case `config` in ('mesh', 'joints', 'uv') for n hands; every array float32 numpy (None: term absent)"""
    p = truth(n, side, seed)
    t = targets_of(p, side, CENTER, root_palm)
    r = M._rng('fit.problem.%s.%s.%d' % (config, side, seed))
    zero = dict.fromkeys(WEIGHTS, 0.0)
    cold = neutral_para(n, 4.0).numpy().astype(np.float32)
    if config == 'mesh':
        return Problem('mesh_' + side, side, CENTER, root_palm, cold, t['verts'], None, None, None, None, dict(zero, w_verts=1e4), (0.03,) * 4)
    if config == 'joints':
        conf = r.uniform(0.2, 1.0, (n, 21)).astype(np.float32)
        jt = t['joints'].copy()
        for i in range(n):
            for j in r.choice(21, 2, replace=False):
                conf[i, j] = 0.0
                jt[i, j] = np.nan
        return Problem('joints_' + side, side, CENTER, root_palm, cold, None, jt, conf, None, None, dict(zero, w_joints=1e4), (0.03,) * 4)
    if config == 'uv':
        init = p.copy()
        init[:, 0:6] += r.normal(0, 0.05, (n, 6)).astype(np.float32)
        init[:, 6:51] += r.normal(0, 0.15, (n, 45)).astype(np.float32)
        init[:, 61:64] += r.normal(0, 0.03, (n, 3)).astype(np.float32)
        conf = np.ones((n, 21), np.float32)
        ut = t['joint_uv'].copy()
        for i in range(n):
            j = int(r.randint(21))
            conf[i, j] = 0.0
            ut[i, j] = np.nan
        return Problem('uv_' + side, side, CENTER, root_palm, init, None, None, None, ut, conf, dict(zero, w_uv=1.0, w_init=1e-3), (0.01, 0.01, 0.0, 0.01))
    raise KeyError(config)


def _finite_rows(*ts):
    ok = None
    for t in ts:
        f = torch.isfinite(t).reshape(t.shape[0], -1).all(1)
        ok = f if ok is None else ok & f
    return ok


def _select(target, conf, dt):
    """(target with unselected entries replaced by 0, selection mask, confidence with unselected entries replaced by 0): selected out, not multiplied by 0"""
    n = target.shape[0]
    conf = torch.ones(n, 21, dtype=dt) if conf is None else conf
    sel = conf > 0
    return torch.where(sel[..., None], target, torch.zeros((), dtype=dt)), sel, torch.where(sel, conf, torch.zeros((), dtype=dt))


def _mse(d, sel=None):
    """per row: mean over the selected entries of |d|^2 (0 where none)"""
    sq = (d * d).sum(-1)
    if sel is None:
        return sq.mean(1)
    cnt = sel.sum(1).to(sq.dtype)
    return torch.where(cnt > 0, torch.where(sel, sq, torch.zeros((), dtype=sq.dtype)).sum(1) / cnt.clamp(min=1), torch.zeros((), dtype=sq.dtype))


def residual_gradient(prob, p, dt, use=None):
    """one evaluation at p [n,64] (dtype dt): -> (g [n,64] = the backward's gradient for the cotangents gV, gJ, gU, before the priors' terms;
    outputs dict verts, joints, joint_uv; mse [n,3]; cotangents dict).  `use` [n] bool: rows whose targets enter (others: no term)."""
    n = p.shape[0]
    T = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dt)  # noqa: E731
    w = prob.weights
    q = p.detach().clone().requires_grad_(True)
    V, J, U, _ = M.mano_outputs(KIND, prob.side, prob.center, q, prob.root_palm, fold=True)
    use = torch.ones(n, dtype=torch.bool) if use is None else use
    zero = torch.zeros((), dtype=dt)
    cot = {'verts': torch.zeros_like(V), 'joints': torch.zeros_like(J), 'joint_uv': torch.zeros_like(U)}
    mse = torch.zeros(n, 3, dtype=dt)
    with torch.no_grad():
        if prob.verts is not None:
            d = V - torch.where(use[:, None, None], T(prob.verts), zero)
            cot['verts'] = torch.where(use[:, None, None], torch.tensor(2.0 * w['w_verts'] / 778.0, dtype=dt) * d, zero)
            mse[:, 0] = torch.where(use, _mse(d), zero)
        if prob.joints is not None:
            t, sel, c = _select(T(prob.joints), T(prob.joints_conf), dt)
            sel = sel & use[:, None]
            d = J - torch.where(sel[..., None], t, zero)
            cot['joints'] = torch.where(sel[..., None], (torch.tensor(2.0 * w['w_joints'] / 21.0, dtype=dt) * c)[..., None] * d, zero)
            mse[:, 1] = _mse(d, sel)
        if prob.joint_uv is not None:
            t, sel, c = _select(T(prob.joint_uv), T(prob.uv_conf), dt)
            sel = sel & use[:, None]
            d = U - torch.where(sel[..., None], t, zero)
            cot['joint_uv'] = torch.where(sel[..., None], (torch.tensor(2.0 * w['w_uv'] / 21.0, dtype=dt) * c)[..., None] * d, zero)
            mse[:, 2] = _mse(d, sel)
    g, = torch.autograd.grad([V, J, U], [q], grad_outputs=[cot['verts'], cot['joints'], cot['joint_uv']])
    return g.detach(), {'verts': V.detach(), 'joints': J.detach(), 'joint_uv': U.detach()}, mse, cot


def adam_step(p, g, m, v, pb1, pb2, lr4, b1, b2, eps):
    """step 5 of the header on [n,64] tensors of one dtype; pb1 / pb2: the running products b1^t, b2^t BEFORE the step -> (p, m, v, pb1, pb2)"""
    dt = p.dtype
    c = lambda x: torch.tensor(x, dtype=dt)  # noqa: E731
    m = c(b1) * m + (c(1.0) - c(b1)) * g
    v = c(b2) * v + (c(1.0) - c(b2)) * (g * g)
    pb1, pb2 = pb1 * c(b1), pb2 * c(b2)
    mhat, vhat = m / (c(1.0) - pb1), v / (c(1.0) - pb2)
    lr = torch.zeros(64, dtype=dt)
    for s, x in zip(GROUP_SLICES, lr4):
        lr[s] = x
    step = (lr * mhat) / (torch.sqrt(vhat) + c(eps))
    return torch.where(lr == 0, p, p - step), m, v, pb1, pb2


def fit(prob, iters, dt=torch.float64, b1=0.9, b2=0.999, eps=1e-8, state=None, anchor=None, init=None):
    """the whole rule on the n rows of `prob` -> dict para, verts, joints, joint_uv, mse_before, mse_after (torch, dtype dt), status (int64 [n]),
    state (m, v, pb1, pb2, t).  state: an earlier result's, to go on from it."""
    p0 = torch.from_numpy(np.asarray(prob.init if init is None else init)).to(dt)
    n = p0.shape[0]
    a = p0 if anchor is None else torch.from_numpy(np.asarray(anchor)).to(dt)
    c = lambda x: torch.tensor(x, dtype=dt)  # noqa: E731
    w = prob.weights
    if state is None:
        m, v, pb1, pb2, t = torch.zeros(n, 64, dtype=dt), torch.zeros(n, 64, dtype=dt), torch.ones(n, 1, dtype=dt), torch.ones(n, 1, dtype=dt), torch.zeros(n, dtype=torch.int64)
    else:
        m, v, pb1, pb2, t = (x.clone() for x in state)
    # status bit 1: p0 / anchor non-finite, or a target in use non-finite
    ok = _finite_rows(p0, a)
    p0_ok = ok.clone()
    T = lambda x: torch.from_numpy(np.asarray(x)).to(dt)  # noqa: E731
    if prob.verts is not None:
        ok &= _finite_rows(T(prob.verts))
    for tg, cf in ((prob.joints, prob.joints_conf), (prob.joint_uv, prob.uv_conf)):
        if tg is not None:
            cf = torch.ones(n, 21, dtype=dt) if cf is None else T(cf)
            sel = cf > 0
            ok &= (~sel | (torch.isfinite(T(tg)).all(-1) & torch.isfinite(cf))).all(1)
    status = torch.where(ok, 0, 2)
    active = ok.clone()
    p = torch.where(p0_ok[:, None], p0, torch.zeros((), dtype=dt))                    # a non-finite row is evaluated nowhere: its outputs are 0
    mse_before = None
    for it in range(iters + 1):
        g, out, mse, _ = residual_gradient(prob, p, dt, use=ok)
        if it == 0:
            mse_before = mse
        if it == iters or not bool(active.any()):
            break
        g[:, 6:51] = g[:, 6:51] + c(2.0 * w['w_pca']) * p[:, 6:51]
        g[:, 51:61] = g[:, 51:61] + c(2.0 * w['w_beta']) * p[:, 51:61]
        g = g + c(2.0 * w['w_init']) * (p - a)
        pn, mn, vn, pb1n, pb2n = adam_step(p, g, m, v, pb1, pb2, prob.lr, b1, b2, eps)
        fin = _finite_rows(pn, mn, vn)
        status = torch.where(active & ~fin, status | 4, status)
        take = active & fin
        active = take
        p, m, v = (torch.where(take[:, None], x, y) for x, y in ((pn, p), (mn, m), (vn, v)))
        pb1, pb2 = torch.where(take[:, None], pb1n, pb1), torch.where(take[:, None], pb2n, pb2)
        t = t + take.to(torch.int64)
    if not bool(active.any()) and iters > 0:
        g, out, mse, _ = residual_gradient(prob, p, dt, use=ok)
    with torch.no_grad():
        R = M.robust_rot6d(p[:, :6])
        status = status | torch.where(p0_ok & (torch.linalg.det(R) < 0), 1, 0)
    z = torch.zeros((), dtype=dt)
    res = {k: torch.where(p0_ok.reshape(-1, *([1] * (o.dim() - 1))), o, z) for k, o in out.items()}
    res.update(para=torch.where(ok[:, None], p, p0), mse_before=torch.where(p0_ok[:, None], mse_before, z), mse_after=torch.where(p0_ok[:, None], mse, z),
               status=status, state=(m, v, pb1, pb2, t))
    return res


def measure(config, iters_list=ITERS, n=3, sides=('right', 'left'), threads=(1, 4)):
    """{iters: {output: largest |float32 run - float64 run|}} of the restatement on problem(config, n, side), both sides.  The float32 run's rounding
    depends on how torch blocks its sums, which changes with the thread count: the larger of the runs at `threads` threads is taken."""
    out = {}
    before = torch.get_num_threads()
    try:
        for nt in threads:
            torch.set_num_threads(nt)
            for side in sides:
                prob = problem(config, n, side)
                for it in iters_list:
                    r32, r64 = fit(prob, it, torch.float32), fit(prob, it, torch.float64)
                    d = out.setdefault(it, dict.fromkeys(OUTPUTS, 0.0))
                    for k in OUTPUTS:
                        d[k] = max(d[k], float((r32[k].double() - r64[k]).abs().max()))
    finally:
        torch.set_num_threads(before)
    return out


# Recorded from measure() on a CPU (torch 2.x, float32 against float64 runs of THIS restatement; never the kernel).  tests/test_mano_fit_ref.py
# re-measures every entry and fails where a re-measured figure exceeds its record.
GATES = {
    'mesh': {
        1: {'para': 4.7e-09, 'verts': 3.37e-08, 'joints': 2.29e-08, 'joint_uv': 9.13e-08, 'mse_after': 2.14e-10},
        2: {'para': 1.75e-07, 'verts': 5.41e-08, 'joints': 2.99e-08, 'joint_uv': 1.19e-07, 'mse_after': 1.4e-09},
        10: {'para': 8.66e-07, 'verts': 1.54e-07, 'joints': 8.01e-08, 'joint_uv': 3.21e-07, 'mse_after': 5.2e-10},
        50: {'para': 6.62e-07, 'verts': 3.9e-08, 'joints': 2e-08, 'joint_uv': 8e-08, 'mse_after': 4.92e-11},
    },
    'joints': {
        1: {'para': 5.07e-09, 'verts': 3.24e-08, 'joints': 3.24e-08, 'joint_uv': 1.3e-07, 'mse_after': 8.42e-11},
        2: {'para': 1.24e-07, 'verts': 5.02e-08, 'joints': 3.68e-08, 'joint_uv': 1.41e-07, 'mse_after': 4.15e-10},
        10: {'para': 7.51e-07, 'verts': 1.47e-07, 'joints': 9.15e-08, 'joint_uv': 3.66e-07, 'mse_after': 3.52e-10},
        50: {'para': 1.01e-06, 'verts': 4.15e-08, 'joints': 1.99e-08, 'joint_uv': 7.93e-08, 'mse_after': 1.23e-11},
    },
    'uv': {
        1: {'para': 6.57e-08, 'verts': 2.64e-08, 'joints': 1.5e-08, 'joint_uv': 7.76e-08, 'mse_after': 1.65e-09},
        2: {'para': 2.43e-07, 'verts': 3.41e-08, 'joints': 2.51e-08, 'joint_uv': 1.03e-07, 'mse_after': 5.65e-09},
        10: {'para': 4.53e-07, 'verts': 4.24e-08, 'joints': 2.88e-08, 'joint_uv': 1.44e-07, 'mse_after': 3.57e-09},
        50: {'para': 6.25e-07, 'verts': 3.48e-08, 'joints': 2.16e-08, 'joint_uv': 8.17e-08, 'mse_after': 8.77e-11},
    },
}


def gate(config, iters, output):
    """the GPU test's bound on |kernel - float64 restatement|: MARGIN x the recorded float32-against-float64 difference"""
    return MARGIN * GATES[config][iters][output]
