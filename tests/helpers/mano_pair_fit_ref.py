"""TEST INFRASTRUCTURE (CPU only: torch CPU): the rule of dir_mano_fit_pair (include/dir_hip.h, "MANO fitting: two hands together") restated in torch,
parametrised by dtype.  Each hand's problem, residual gradient and Adam step are mano_fit_ref's; the closest points of two segments (Ericson's
procedure, every clamp and the degenerate branches in the header's order), the capsule overlaps h, their envelope gradient (s, t held fixed), the
gather into the joint cotangents and the offset's own terms and Adam group are written out by hand here.  The joint cotangent of the collision
term goes through the MANO layer by autograd, as the residuals' cotangents do in mano_fit_ref.

CANONICAL CASES   pair_problem(config, n), n <= 5: hands from mano_fit_ref (left: seed SEEDS[config], right: that seed + 1) on the 'pca' tables, both
centred at joint 9, the right hand offset by OFFSETS[row] (2 .. 4 cm; at the truth the capsules overlap by 10 .. 18 mm), radii RADII (6 .. 10 mm, the right
hand's in reverse order):
    'separate'  anchor + collision only: start at the truth, w_init 1e-2, w_off_init 1, w_col 1e4; betas and camera frozen     (the behaviour case)
    'joints'    mano_fit_ref's cold 'joints' problem per hand + w_col 1e4 + an offset target with confidence (w_off 10); start o = target + 1 cm
    'uv'        mano_fit_ref's 'uv' refinement per hand + w_col 1e3 + w_off_init 1

GATES   GATES[config][iters][output] = the largest |restatement float32 - restatement float64| over pair_problem(config, 3), recorded here from a
CPU run and re-measured by tests/test_mano_pair_fit_ref.py.  The GPU test allows mano_fit_ref.MARGIN = 4 x the record.  Nothing here is measured on
the kernel.

BRANCH MARGINS   The objective is not smooth where a pair switches on (h = 0) or a clamp of the segment procedure changes, and a float32 run that
takes another branch there is not a rounding difference.  fit_pair records, over every evaluated iterate, H_MARGIN = the smallest |r_i + r_j - d_ij|
over ALL pairs and, over the pairs with h > -1 mm, S_MARGIN = the smallest distance of a clamp's input from 0 and from 1 (the inputs the procedure
actually evaluates) and of |den| / (a e) from 0.  tests/test_mano_pair_fit_ref.py asserts H_MARGIN >= H_MIN and S_MARGIN >= S_MIN on the float64
run of every canonical case over 50 iterations; the cases (seeds, offsets) were chosen on the CPU so that this holds.
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
import mano_fit_ref as R  # noqa: E402

PARENT = (0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19)
CHILD = tuple(range(1, 21))
SEG_EPS, MIN_DIST = 1e-12, 1e-6
ITERS = R.ITERS
OUTPUTS = ('para', 'offset', 'verts', 'joints', 'joint_uv', 'col')
H_MIN, S_MIN = 1e-6, 1e-5          # metres; parameter units.  float32 joints carry ~1e-7 m, a float32 clamp input ~1e-6
NEAR = 1e-3                        # a pair with h > -NEAR counts as nearly active
RADII = tuple(np.float32(0.006 + 0.004 * ((7 * k) % 20) / 19.0) for k in range(20))
OFFSETS = ((0.018, 0.004, 0.008), (-0.022, 0.018, 0.010), (0.012, -0.028, 0.016), (0.026, 0.020, -0.008), (-0.010, -0.008, 0.018))
SEEDS = {'separate': 0, 'joints': 4, 'uv': 2}          # chosen on the CPU so that the branch margins below hold on the float64 runs
CONFIGS = ('separate', 'joints', 'uv')


# ------------------------------------------------------------------------------------------------ the segment procedure
def _clamp01(x):
    return torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))           # NaN stays NaN


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def segments(A, B, C, D):
    """closest points of the segments (A, B) and (C, D) [..., 3] in the tensors' dtype, the header's branches evaluated in its order
    -> dict s, t, d, n and margin (how far the clamp inputs that were evaluated, and den / (a e), stay from a switch)"""
    dt = A.dtype
    d1, d2, r = B - A, D - C, A - C
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    c, b = _dot(d1, r), _dot(d1, d2)
    eps = torch.tensor(SEG_EPS, dtype=dt)
    one, zero, big = torch.ones_like(a), torch.zeros_like(a), torch.full_like(a, 1e30)
    pa, pe = a <= eps, e <= eps
    sa, se = torch.where(pa, one, a), torch.where(pe, one, e)               # divisions of the untaken branches stay finite
    m01 = lambda x: torch.minimum(x.abs(), (x - 1).abs())  # noqa: E731
    # general branch
    den = a * e - b * b
    s_raw = (b * f - c * e) / torch.where(den != 0, den, one)
    s_g = torch.where(den != 0, _clamp01(s_raw), zero)
    t_raw = (b * s_g + f) / se
    s_lo, s_hi = -c / sa, (b - c) / sa
    s_gen = torch.where(t_raw < 0, _clamp01(s_lo), torch.where(t_raw > 1, _clamp01(s_hi), s_g))
    t_gen = _clamp01(t_raw)
    mar_gen = torch.minimum(torch.minimum(m01(t_raw), torch.where(den != 0, m01(s_raw), big)), (den / (sa * se)).abs())
    mar_gen = torch.minimum(mar_gen, torch.where(t_raw < 0, m01(s_lo), torch.where(t_raw > 1, m01(s_hi), big)))
    # the degenerate branches
    t_pa = _clamp01(f / se)
    s_pe = _clamp01(s_lo)
    s = torch.where(pa, zero, torch.where(pe, s_pe, s_gen))
    t = torch.where(pa & pe, zero, torch.where(pa, t_pa, torch.where(pe, zero, t_gen)))
    margin = torch.where(pa & pe, big, torch.where(pa, m01(f / se), torch.where(pe, m01(s_lo), mar_gen)))
    w = (A + s[..., None] * d1) - (C + t[..., None] * d2)
    d = torch.sqrt(_dot(w, w))
    return {'s': s, 't': t, 'd': d, 'n': w / d[..., None], 'margin': margin}


def collision(XL, XR, rL, rR, k_col):
    """the capsule term at the common-frame joints XL, XR [n,21,3]: -> dict h [n,20,20] (0 where skipped), active, nodir [n,20,20] bool,
    gL, gR [n,21,3] (the joint cotangents of step 2a), go [n,3], col [n,2] (sum h^2 / 400, max h), h_margin, s_margin [n]"""
    dt = XL.dtype
    pa, ch = list(PARENT), list(CHILD)
    A, B = XL[:, pa][:, :, None], XL[:, ch][:, :, None]                      # [n,20,1,3]
    C, D = XR[:, pa][:, None], XR[:, ch][:, None]                            # [n,1,20,3]
    A, B, C, D = (x.expand(-1, 20, 20, 3) for x in (A, B, C, D))
    g = segments(A, B, C, D)
    s, t, d, nrm = g['s'], g['t'], g['d'], g['n']
    rsum = rL[:, None] + rR[None, :]
    fin = torch.isfinite(d)
    raw = rsum - d
    pos = fin & (raw > 0)
    zero = torch.zeros((), dtype=dt)
    h = torch.where(pos, raw, zero)
    nodir = ~fin | (pos & (d < MIN_DIST))
    active = pos & ~(d < MIN_DIST)
    u = torch.where(active, torch.as_tensor(k_col, dtype=dt) * h, zero)
    nz = torch.where(active[..., None], nrm, zero)
    gA, gB = -((u * (1 - s))[..., None] * nz), -((u * s)[..., None] * nz)
    gC, gD = (u * (1 - t))[..., None] * nz, (u * t)[..., None] * nz
    n = XL.shape[0]
    gL, gR = torch.zeros(n, 21, 3, dtype=dt), torch.zeros(n, 21, 3, dtype=dt)
    GA, GB, GC, GD = gA.sum(2), gB.sum(2), gC.sum(1), gD.sum(1)              # per left bone over j, per right bone over i
    for k in range(20):                                                      # bone-index order per joint
        gL[:, PARENT[k]] = gL[:, PARENT[k]] + GA[:, k]
        gL[:, CHILD[k]] = gL[:, CHILD[k]] + GB[:, k]
        gR[:, PARENT[k]] = gR[:, PARENT[k]] + GC[:, k]
        gR[:, CHILD[k]] = gR[:, CHILD[k]] + GD[:, k]
    go = (gC + gD).sum(2).sum(1)
    col = torch.stack([(h * h).sum(2).sum(1) / 400, h.reshape(n, -1).max(1).values], 1)
    near = fin & (raw > -NEAR)
    big = torch.full_like(d, 1e30)
    return {'h': h, 'active': active, 'nodir': nodir, 'gL': gL, 'gR': gR, 'go': go, 'col': col, 'd': d, 's': s, 't': t,
            'h_margin': torch.where(fin, raw.abs(), big).reshape(n, -1).min(1).values,
            's_margin': torch.where(near, g['margin'], big).reshape(n, -1).min(1).values}


# ------------------------------------------------------------------------------------------------ the canonical cases
PairProblem = collections.namedtuple('PairProblem', 'name hands o0 o_target o_conf o_anchor radii pair_weights lr_o')


def radii_np():
    return np.asarray(RADII, np.float32)


def pair_problem(config, n, seed=None):
    """the canonical pair case `config` for n pairs (n <= 5): hands = (left Problem, right Problem) of mano_fit_ref with ONE set of weights and rates"""
    seed = SEEDS[config] if seed is None else seed
    o = np.asarray(OFFSETS[:n], np.float32)
    rad = (radii_np(), radii_np()[::-1].copy())
    zero = dict.fromkeys(R.WEIGHTS, 0.0)
    if config == 'separate':
        hs = []
        for side, sd in (('left', seed), ('right', seed + 1)):
            p = R.truth(n, side, sd)
            hs.append(R.Problem('separate_' + side, side, R.CENTER, False, p, None, None, None, None, None, dict(zero, w_init=1e-2), (0.01, 0.01, 0.0, 0.0)))
        return PairProblem('separate', tuple(hs), o, None, None, None, rad, {'w_col': 1e4, 'w_off': 0.0, 'w_off_init': 1.0}, 3e-3)
    if config == 'joints':
        hs = (R.problem('joints', n, 'left', seed), R.problem('joints', n, 'right', seed + 1))
        conf = np.linspace(0.5, 1.0, n).astype(np.float32)
        return PairProblem('joints', hs, (o + np.float32(0.01)).astype(np.float32), o, conf, None, rad, {'w_col': 1e4, 'w_off': 10.0, 'w_off_init': 0.0}, 3e-3)
    if config == 'uv':
        hs = (R.problem('uv', n, 'left', seed), R.problem('uv', n, 'right', seed + 1))
        return PairProblem('uv', hs, o, None, None, None, rad, {'w_col': 1e3, 'w_off': 0.0, 'w_off_init': 1.0}, 2e-3)
    raise KeyError(config)


# ------------------------------------------------------------------------------------------------ the rule
def _extra_gradient(prob, p, dt, gj):
    """the MANO backward of a joint cotangent gj [n,21,3] at p"""
    q = p.detach().clone().requires_grad_(True)
    _, J, _, _ = M.mano_outputs(R.KIND, prob.side, prob.center, q, prob.root_palm, fold=True)
    g, = torch.autograd.grad([J], [q], grad_outputs=[gj])
    return g.detach()


def _adam3(o, g, m, v, pb1, pb2, lr, b1, b2, eps):
    dt = o.dtype
    c = lambda x: torch.tensor(x, dtype=dt)  # noqa: E731
    m = c(b1) * m + (c(1.0) - c(b1)) * g
    v = c(b2) * v + (c(1.0) - c(b2)) * (g * g)
    pb1, pb2 = pb1 * c(b1), pb2 * c(b2)
    step = (c(lr) * (m / (c(1.0) - pb1))) / (torch.sqrt(v / (c(1.0) - pb2)) + c(eps))
    return (o if lr == 0 else o - step), m, v, pb1, pb2


def _hand_ok(prob, p0, a, dt):
    """(not passed through, p0 and anchor finite) per row: dir_mano_fit's status bit 1"""
    n = p0.shape[0]
    ok = R._finite_rows(p0, a)
    p0_ok = ok.clone()
    T = lambda x: torch.from_numpy(np.asarray(x)).to(dt)  # noqa: E731
    if prob.verts is not None:
        ok &= R._finite_rows(T(prob.verts))
    for tg, cf in ((prob.joints, prob.joints_conf), (prob.joint_uv, prob.uv_conf)):
        if tg is not None:
            cf = torch.ones(n, 21, dtype=dt) if cf is None else T(cf)
            sel = cf > 0
            ok &= (~sel | (torch.isfinite(T(tg)).all(-1) & torch.isfinite(cf))).all(1)
    return ok, p0_ok


def fit_pair(pp, iters, dt=torch.float64, b1=0.9, b2=0.999, eps=1e-8, state=None, init=None, anchor=None, o0=None):
    """the whole rule on the n pairs of `pp` -> dict: hands (two dicts as mano_fit_ref.fit's), offset [n,3], col [n,4], pair_status [n], state
    (per hand (m, v, pb1, pb2, t), then the offset's), h_margin, s_margin (the smallest over every evaluated iterate and pair)"""
    T = lambda x: torch.from_numpy(np.asarray(x)).to(dt)  # noqa: E731
    c = lambda x: torch.tensor(x, dtype=dt)  # noqa: E731
    zero = torch.zeros((), dtype=dt)
    hs = pp.hands
    p0 = [T(h.init if init is None else init[i]) for i, h in enumerate(hs)]
    n = p0[0].shape[0]
    an = [p0[i] if anchor is None else T(anchor[i]) for i in range(2)]
    oo0 = T(pp.o0 if o0 is None else o0)
    oa = oo0 if pp.o_anchor is None else T(pp.o_anchor)
    use_t = torch.zeros(n, dtype=torch.bool)
    co, ot = torch.zeros(n, dtype=dt), torch.zeros(n, 3, dtype=dt)
    if pp.o_target is not None:
        cf = torch.ones(n, dtype=dt) if pp.o_conf is None else T(pp.o_conf)
        use_t = cf > 0
        co, ot = torch.where(use_t, cf, zero), torch.where(use_t[:, None], T(pp.o_target), zero)
    rad = [T(r) for r in pp.radii]
    okp = [_hand_ok(h, p0[i], an[i], dt) for i, h in enumerate(hs)]
    ok, p0_ok = [x[0] for x in okp], [x[1] for x in okp]
    any_pass = ~(ok[0] & ok[1])
    o_bad = ~(R._finite_rows(oo0, oa, ot) & torch.isfinite(co) & bool(torch.isfinite(rad[0]).all() and torch.isfinite(rad[1]).all()))
    coupled = ~any_pass & ~o_bad
    pstatus = torch.where(any_pass, 1, 0) | torch.where(o_bad, 2, 0)
    if state is None:
        st = [(torch.zeros(n, 64, dtype=dt), torch.zeros(n, 64, dtype=dt), torch.ones(n, 1, dtype=dt), torch.ones(n, 1, dtype=dt), torch.zeros(n, dtype=torch.int64))
              for _ in range(2)]
        sto = (torch.zeros(n, 3, dtype=dt), torch.zeros(n, 3, dtype=dt), torch.ones(n, 1, dtype=dt), torch.ones(n, 1, dtype=dt), torch.zeros(n, dtype=torch.int64))
    else:
        st, sto = [tuple(x.clone() for x in s) for s in state[:2]], tuple(x.clone() for x in state[2])
    p = [torch.where(p0_ok[i][:, None], p0[i], zero) for i in range(2)]
    o = torch.where(coupled[:, None], oo0, zero)
    status = [torch.where(ok[i], 0, 2) for i in range(2)]
    alive = [ok[i].clone() for i in range(2)]
    o_alive = coupled.clone()
    k_col = float(np.float32(2.0 * pp.pair_weights.get('w_col', 0.0) / 400.0)) if dt == torch.float32 else 2.0 * pp.pair_weights.get('w_col', 0.0) / 400.0
    k_off, k_oi = 2.0 * pp.pair_weights.get('w_off', 0.0), 2.0 * pp.pair_weights.get('w_off_init', 0.0)
    col = torch.zeros(n, 4, dtype=dt)
    h_margin, s_margin = torch.full((n,), 1e30, dtype=dt), torch.full((n,), 1e30, dtype=dt)
    mse0 = [None, None]
    for it in range(iters + 1):
        ev = [R.residual_gradient(hs[i], p[i], dt, use=ok[i]) for i in range(2)]
        cl = collision(ev[0][1]['joints'], ev[1][1]['joints'] + o[:, None], rad[0], rad[1], k_col)
        h_margin = torch.minimum(h_margin, torch.where(coupled, cl['h_margin'], h_margin))
        s_margin = torch.minimum(s_margin, torch.where(coupled, cl['s_margin'], s_margin))
        if it == 0:
            mse0 = [e[2] for e in ev]
            col[:, :2] = torch.where(coupled[:, None], cl['col'], zero)
        if it == 0 or it == iters:
            pstatus = pstatus | torch.where(coupled & cl['nodir'].reshape(n, -1).any(1), 8, 0)
        if it == iters:
            col[:, 2:] = torch.where(coupled[:, None], cl['col'], zero)
            break
        grad_col = coupled & (k_col > 0)
        pstatus = pstatus | torch.where(grad_col & cl['nodir'].reshape(n, -1).any(1), 8, 0)
        for i in range(2):
            g = ev[i][0]
            gj = torch.where(grad_col[:, None, None], cl['gL' if i == 0 else 'gR'], zero)
            g = g + _extra_gradient(hs[i], p[i], dt, gj)
            w = hs[i].weights
            g[:, 6:51] = g[:, 6:51] + c(2.0 * w['w_pca']) * p[i][:, 6:51]
            g[:, 51:61] = g[:, 51:61] + c(2.0 * w['w_beta']) * p[i][:, 51:61]
            g = g + c(2.0 * w['w_init']) * (p[i] - an[i])
            m, v, pb1, pb2, t = st[i]
            pn, mn, vn, pb1n, pb2n = R.adam_step(p[i], g, m, v, pb1, pb2, hs[i].lr, b1, b2, eps)
            fin = R._finite_rows(pn, mn, vn)
            status[i] = torch.where(alive[i] & ~fin, status[i] | 4, status[i])
            take = alive[i] & fin
            alive[i] = take
            p[i], m, v = (torch.where(take[:, None], x, y) for x, y in ((pn, p[i]), (mn, m), (vn, v)))
            st[i] = (m, v, torch.where(take[:, None], pb1n, pb1), torch.where(take[:, None], pb2n, pb2), t + take.to(torch.int64))
        g = torch.where(grad_col[:, None], cl['go'], zero)
        g = g + torch.where(use_t[:, None], (c(k_off) * co)[:, None] * (o - ot), zero)
        g = g + c(k_oi) * (o - oa)
        m, v, pb1, pb2, t = sto
        on, mn, vn, pb1n, pb2n = _adam3(o, g, m, v, pb1, pb2, pp.lr_o, b1, b2, eps)
        fin = R._finite_rows(on, mn, vn)
        pstatus = torch.where(o_alive & ~fin, pstatus | 4, pstatus)
        take = o_alive & fin
        o_alive = take
        o, m, v = (torch.where(take[:, None], x, y) for x, y in ((on, o), (mn, m), (vn, v)))
        sto = (m, v, torch.where(take[:, None], pb1n, pb1), torch.where(take[:, None], pb2n, pb2), t + take.to(torch.int64))
    hands = []
    for i in range(2):
        out, mse = ev[i][1], ev[i][2]
        with torch.no_grad():
            Rm = M.robust_rot6d(p[i][:, :6])
            stt = status[i] | torch.where(p0_ok[i] & (torch.linalg.det(Rm) < 0), 1, 0)
        res = {k: torch.where(p0_ok[i].reshape(-1, *([1] * (x.dim() - 1))), x, zero) for k, x in out.items()}
        res.update(para=torch.where(ok[i][:, None], p[i], p0[i]), mse_before=torch.where(p0_ok[i][:, None], mse0[i], zero),
                   mse_after=torch.where(p0_ok[i][:, None], mse, zero), status=stt)
        hands.append(res)
    return {'hands': hands, 'offset': torch.where(coupled[:, None], o, oo0), 'col': col, 'pair_status': pstatus, 'state': (st[0], st[1], sto),
            'h_margin': h_margin, 's_margin': s_margin}


def flat(res):
    """the outputs the gates are recorded for: both hands stacked"""
    out = {k: torch.stack([res['hands'][0][k], res['hands'][1][k]]) for k in ('para', 'verts', 'joints', 'joint_uv')}
    out.update(offset=res['offset'], col=res['col'])
    return out


def energy(pp, p, o, dt=torch.float64, detach_st=True):
    """the one-scalar objective E summed over the pairs at p = [p_L, p_R] (tensors that may require grad) and o; with detach_st the closest-point
    parameters s, t are constants (the envelope gradient's objective)"""
    T = lambda x: torch.from_numpy(np.asarray(x)).to(dt)  # noqa: E731
    E = torch.zeros((), dtype=dt)
    X = []
    for i, h in enumerate(pp.hands):
        V, J, U, _ = M.mano_outputs(R.KIND, h.side, h.center, p[i], h.root_palm, fold=True)
        X.append(J)
        w = h.weights
        n = p[i].shape[0]
        if h.verts is not None:
            E = E + w['w_verts'] / 778.0 * ((V - T(h.verts)) ** 2).sum()
        if h.joints is not None:
            t, sel, cf = R._select(T(h.joints), None if h.joints_conf is None else T(h.joints_conf), dt)
            E = E + w['w_joints'] / 21.0 * (cf[..., None] * torch.where(sel[..., None], (J - t) ** 2, torch.zeros((), dtype=dt))).sum()
        if h.joint_uv is not None:
            t, sel, cf = R._select(T(h.joint_uv), None if h.uv_conf is None else T(h.uv_conf), dt)
            E = E + w['w_uv'] / 21.0 * (cf[..., None] * torch.where(sel[..., None], (U - t) ** 2, torch.zeros((), dtype=dt))).sum()
        a = T(h.init)
        E = E + w['w_pca'] * (p[i][:, 6:51] ** 2).sum() + w['w_beta'] * (p[i][:, 51:61] ** 2).sum() + w['w_init'] * ((p[i] - a) ** 2).sum()
        del n
    pw = pp.pair_weights
    if pp.o_target is not None:
        cf = torch.ones(o.shape[0], dtype=dt) if pp.o_conf is None else T(pp.o_conf)
        E = E + pw.get('w_off', 0.0) * (torch.where(cf > 0, cf, torch.zeros((), dtype=dt))[:, None] * (o - T(pp.o_target)) ** 2).sum()
    E = E + pw.get('w_off_init', 0.0) * ((o - T(pp.o0 if pp.o_anchor is None else pp.o_anchor)) ** 2).sum()
    XL, XR = X[0], X[1] + o[:, None]
    pa, ch = list(PARENT), list(CHILD)
    A, B = XL[:, pa][:, :, None].expand(-1, 20, 20, 3), XL[:, ch][:, :, None].expand(-1, 20, 20, 3)
    C, D = XR[:, pa][:, None].expand(-1, 20, 20, 3), XR[:, ch][:, None].expand(-1, 20, 20, 3)
    if detach_st:
        with torch.no_grad():
            g = segments(A, B, C, D)
        s, t = g['s'][..., None], g['t'][..., None]
        wv = (A + s * (B - A)) - (C + t * (D - C))
        d = torch.sqrt(_dot(wv, wv))
    else:
        d = segments(A, B, C, D)['d']
    h = torch.clamp((T(pp.radii[0])[:, None] + T(pp.radii[1])[None, :]) - d, min=0)
    return E + pw.get('w_col', 0.0) / 400.0 * (h * h).sum()


def measure(config, iters_list=ITERS, n=3, threads=(1, 4)):
    """{iters: {output: largest |float32 run - float64 run|}} of the restatement on pair_problem(config, n); the larger of the runs at `threads` threads"""
    out = {}
    before = torch.get_num_threads()
    try:
        for nt in threads:
            torch.set_num_threads(nt)
            pp = pair_problem(config, n)
            for it in iters_list:
                r32, r64 = flat(fit_pair(pp, it, torch.float32)), flat(fit_pair(pp, it, torch.float64))
                d = out.setdefault(it, dict.fromkeys(OUTPUTS, 0.0))
                for k in OUTPUTS:
                    d[k] = max(d[k], float((r32[k].double() - r64[k]).abs().max()))
    finally:
        torch.set_num_threads(before)
    return out


# Recorded from measure() on a CPU (torch 2.x, float32 against float64 runs of THIS restatement; never the kernel).  tests/test_mano_pair_fit_ref.py
# re-measures every entry and fails where a re-measured figure exceeds its record.
GATES = {
    'separate': {
        1: {'para': 5.66e-08, 'offset': 5.22e-10, 'verts': 2.78e-08, 'joints': 1.54e-08, 'joint_uv': 6.87e-08, 'col': 5.94e-09},
        2: {'para': 9.38e-08, 'offset': 1.78e-08, 'verts': 3.14e-08, 'joints': 2.56e-08, 'joint_uv': 8.97e-08, 'col': 2.66e-08},
        10: {'para': 2.61e-07, 'offset': 5.29e-08, 'verts': 4.91e-08, 'joints': 3.08e-08, 'joint_uv': 1.12e-07, 'col': 5.94e-09},
        50: {'para': 1.62e-07, 'offset': 2.84e-08, 'verts': 3.21e-08, 'joints': 1.46e-08, 'joint_uv': 4.84e-08, 'col': 5.94e-09},
    },
    'joints': {
        1: {'para': 6.26e-09, 'offset': 8.28e-10, 'verts': 2.89e-08, 'joints': 2.09e-08, 'joint_uv': 8.32e-08, 'col': 2.68e-09},
        2: {'para': 1.17e-06, 'offset': 9.77e-09, 'verts': 7.2e-08, 'joints': 4.3e-08, 'joint_uv': 1.73e-07, 'col': 1.84e-09},
        10: {'para': 1.39e-06, 'offset': 3.05e-08, 'verts': 2.06e-07, 'joints': 1.7e-07, 'joint_uv': 6.76e-07, 'col': 1.07e-07},
        50: {'para': 1.44e-06, 'offset': 2.22e-08, 'verts': 4.45e-08, 'joints': 2.43e-08, 'joint_uv': 9.68e-08, 'col': 1.94e-08},
    },
    'uv': {
        1: {'para': 1.71e-07, 'offset': 5.5e-10, 'verts': 3.07e-08, 'joints': 1.13e-08, 'joint_uv': 5.63e-08, 'col': 9.16e-09},
        2: {'para': 3.81e-07, 'offset': 6.35e-09, 'verts': 2.96e-08, 'joints': 1.57e-08, 'joint_uv': 8.45e-08, 'col': 1.01e-08},
        10: {'para': 5.33e-07, 'offset': 2.36e-08, 'verts': 4.78e-08, 'joints': 3.69e-08, 'joint_uv': 1.66e-07, 'col': 1.34e-08},
        50: {'para': 5.49e-07, 'offset': 1.11e-08, 'verts': 3.13e-08, 'joints': 2.62e-08, 'joint_uv': 9.36e-08, 'col': 9e-09},
    },
}


def gate(config, iters, output):
    """the GPU test's bound on |kernel - float64 restatement|: MARGIN x the recorded float32-against-float64 difference"""
    return R.MARGIN * GATES[config][iters][output]
