"""TEST INFRASTRUCTURE (CPU only: torch CPU): the rule of dir_mano_fit_start (include/dir_hip.h, "MANO fitting: closed-form start") restated in torch,
parametrised by dtype, on top of mano_cases.mano_outputs in the kernels' order (fold=True).  Horn's rotation is restated with the kernel's own
cyclic Jacobi procedure (csrc/horn_rotation.h), by dtype, so that a float32 run is representative of float32 arithmetic.

CASES   tables synth.mano_buffers (table set 'pca'); `far_truth(n, side, lo, hi)` = mano_fit_ref.truth's hands with the root angle drawn from [lo, hi] rad;
the start is neutral_para(n, 4) (zero betas: the truth's differ), every case 3 rows x both sides:
    'mesh'        vertices (w_verts 1e4), root angle 1.8 .. 3.1
    'joints'      3-D joints with confidences in (0.2, 1], joints 5 (rigid) and 11 at confidence 0 holding NaN (w_joints 1e4), 2.6 .. 3.14
    'all'         vertices + joints + 2-D keypoints, one keypoint per hand at confidence 0 holding NaN, 1.8 .. 3.1
    'uv'          2-D keypoints alone: the search over the cube's rotations, 2.6 .. 3.14
    'centre-1'    vertices + joints + 2-D keypoints with center_idx -1 (the pivot is the rest-pose wrist), 1.8 .. 3.1
    'root_palm'   joints + 2-D keypoints with the root_palm wrist (joint 0 is not rigid), 1.8 .. 3.1
Seeds: every 2-D-only problem used by a test (CASES 'uv', the value test's, the GPU tests') was checked for the float64 gap between the best and the
second-best e_k: tests/test_mano_start_ref.py asserts it is at least 1e-3 of the best, so a float32 run cannot pick another candidate.  Seed 0
satisfies it everywhere it is used.

GATES   GATES[case][output] = the largest |restatement float32 - restatement float64| over CASES (3 rows, both sides; the larger of the runs at 1 and 4
torch threads): 'root' the angle between the two roots (rad), 'cam' the three camera scalars, 'info' relative to the float64 value.  Recorded here
from a CPU run, re-measured by tests/test_mano_start_ref.py, which fails where a re-measured figure exceeds its record.  The GPU test allows
MARGIN = 4 x the record (the project's margin for another valid summation order).  Nothing here is measured on the kernel.

VALUE   what the start buys the fit (mano_fit_ref.fit in float64 from the cold and from the started parameters, 4 rows per case), recorded from
tests/test_mano_start_ref.py's value test, which prints the figures and fails where a row's started fit is not below its cold fit.
"""
import itertools
import os
import sys

import numpy as np
import torch

_here = os.path.dirname(os.path.abspath(__file__))
if _here not in sys.path:
    sys.path.insert(0, _here)
import mano_cases as M  # noqa: E402
import mano_fit_ref as R  # noqa: E402

KIND = R.KIND
RS = (0, 1, 5, 9, 13, 17)
MARGIN = 4.0
JACOBI_SWEEPS = 12
CASE_NAMES = ('mesh', 'joints', 'all', 'uv', 'centre-1', 'root_palm')
OUTPUTS = ('root', 'cam', 'info')


# ===================================================================================================================== the candidates
def cube_rotations():
    """the 24 proper rotations of the cube in the header's order: [24,3,3] int64 numpy, row r has sg[r] at column perm[r]"""
    out = []
    for perm in itertools.permutations((0, 1, 2)):                   # lexicographic
        for sg in itertools.product((1, -1), repeat=3):             # (+,+,+), (+,+,-), (+,-,+), ...
            P = np.zeros((3, 3), np.int64)
            for r in range(3):
                P[r, perm[r]] = sg[r]
            if round(np.linalg.det(P)) == 1:
                out.append(P)
    return np.stack(out)


# ===================================================================================================================== Horn's rotation
def _jacobi_rotate(a, v, P, Q):
    """csrc/horn_rotation.h jacobi_rotate on lists of lists of [n] tensors; rows whose a[P][Q] is exactly 0 are left as they are"""
    apq = a[P][Q]
    skip = apq == 0
    one = torch.ones_like(apq)
    safe = torch.where(skip, one, apq)
    theta = (a[Q][Q] - a[P][P]) / (2.0 * safe)
    t = torch.copysign(one, theta) / (theta.abs() + torch.sqrt(theta * theta + 1.0))
    c = 1.0 / torch.sqrt(t * t + 1.0)
    s = t * c
    tau = s / (1.0 + c)
    keep = lambda new, old: torch.where(skip, old, new)  # noqa: E731
    zero = torch.zeros_like(apq)
    a[P][P], a[Q][Q] = keep(a[P][P] - t * apq, a[P][P]), keep(a[Q][Q] + t * apq, a[Q][Q])
    a[P][Q] = a[Q][P] = keep(zero, apq)
    for r in range(4):
        if r != P and r != Q:
            g, h = a[r][P], a[r][Q]
            a[r][P] = a[P][r] = keep(g - s * (h + g * tau), g)
            a[r][Q] = a[Q][r] = keep(h + s * (g - h * tau), h)
    for r in range(4):
        g, h = v[r][P], v[r][Q]
        v[r][P] = keep(g - s * (h + g * tau), g)
        v[r][Q] = keep(h + s * (g - h * tau), h)


def horn_rotation(S):
    """S [n,3,3] (S[a][b] = sum p_a g_b) -> the proper rotation [n,3,3] that maximises sum g . R p, by the kernel's procedure in S's dtype"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (S[:, i, j] for i in range(3) for j in range(3))
    a = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]]
    one, zero = torch.ones_like(Sxx), torch.zeros_like(Sxx)
    v = [[one if i == j else zero for j in range(4)] for i in range(4)]
    m = torch.stack([a[i][j].abs() for i in range(4) for j in range(4)]).amax(0)
    inv = torch.where(m > 0, 1.0 / torch.where(m > 0, m, one), one)
    a = [[a[i][j] * inv for j in range(4)] for i in range(4)]
    for _ in range(JACOBI_SWEEPS):
        off = sum(a[i][j].abs() for i in range(4) for j in range(i + 1, 4))
        if not bool((off != 0).any()):
            break
        for P, Q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _jacobi_rotate(a, v, P, Q)
    best, w, x, y, z = a[0][0], v[0][0], v[1][0], v[2][0], v[3][0]
    for k in range(1, 4):
        take = a[k][k] > best
        best = torch.where(take, a[k][k], best)
        w, x, y, z = (torch.where(take, v[i][k], q) for i, q in enumerate((w, x, y, z)))
    n = 1.0 / torch.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w * n, x * n, y * n, z * n
    return torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                        2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                        2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], 1).reshape(-1, 3, 3)


# ===================================================================================================================== the rule
def camera_fit(X, U, d):
    """step 4 on X [n,21,2], U [n,21,2], d [n,21] (0 where selected out) -> s [n], t [n,2], residual [n], denominator [n]"""
    D = d.sum(1)
    Xm, Um = (d[..., None] * X).sum(1) / D[:, None], (d[..., None] * U).sum(1) / D[:, None]
    dx, du = X - Xm[:, None], U - Um[:, None]
    num, den = (d * (dx * du).sum(-1)).sum(1), (d * (dx * dx).sum(-1)).sum(1)
    s = num / den
    t = Um - s[:, None] * Xm
    return s, t, residual_uv(X, U, d, s, t), den


def residual_uv(X, U, d, s, t):
    r = s[:, None, None] * X + t[:, None] - U
    return (d * (r * r).sum(-1)).sum(1)


def start(prob, dt=torch.float64, root=True, cam=True, search=True, init=None):
    """the whole rule on the n rows of `prob` (a mano_fit_ref.Problem; its weights' w_verts and w_joints are read) -> dict para [n,64], status, choice
    (int64 [n]), info [n,4], R1 [n,3,3] (the root written, R0 where kept), e_k [n,24] (inf where dropped or no search ran)"""
    T = lambda x: torch.from_numpy(np.asarray(x)).to(dt)  # noqa: E731
    zero = torch.zeros((), dtype=dt)
    p0 = T(prob.init if init is None else init)
    n = p0.shape[0]
    kv = torch.tensor(float(np.float32(prob.weights.get('w_verts', 0.0) / 778.0)), dtype=dt)
    kj = torch.tensor(float(np.float32(prob.weights.get('w_joints', 0.0) / 21.0)), dtype=dt)
    # ---- step 0
    p0_ok = torch.isfinite(p0).all(1)
    ok = p0_ok.clone()
    if prob.verts is not None:
        ok &= torch.isfinite(T(prob.verts)).reshape(n, -1).all(1)
    sel = {}
    for name, tg, cf in (('j', prob.joints, prob.joints_conf), ('u', prob.joint_uv, prob.uv_conf)):
        if tg is not None:
            cf = torch.ones(n, 21, dtype=dt) if cf is None else T(cf)
            s_ = cf > 0
            ok &= (~s_ | (torch.isfinite(T(tg)).all(-1) & torch.isfinite(cf))).all(1)
            sel[name] = (s_, cf)
    p = torch.where(p0_ok[:, None], p0, R.neutral_para(n, 1.0, dt))
    with torch.no_grad():
        R0 = M.robust_rot6d(p[:, :6])
        reflect = p0_ok & (torch.linalg.det(R0.double()) < 0)
        V, J, _, _ = M.mano_outputs(KIND, prob.side, prob.center, p, prob.root_palm, fold=True)
    use = ok & ~reflect
    # ---- step 1
    if prob.center >= 0:
        pi = torch.zeros(n, 3, dtype=dt)
    else:
        tt = M._tt(KIND, prob.side, dt)
        pi = torch.einsum('ck,bk->bc', tt['j_shapedirs'][0], p[:, 51:61]) + tt['j_template'][0]
    have3d = prob.verts is not None or prob.joints is not None
    status = torch.where(ok, 0, 2) | torch.where(reflect, 1, 0)
    info = torch.zeros(n, 4, dtype=dt)
    R1 = R0.clone()
    new_root = torch.zeros(n, dtype=torch.bool)
    # ---- step 2
    Y = J
    if have3d and root:
        xs, ys, ws = [], [], []
        if prob.joints is not None:
            s_, cf = sel['j']
            rigid = torch.zeros(21, dtype=torch.bool)
            rigid[[j for j in RS if not (j == 0 and prob.root_palm)]] = True
            s_ = s_ & rigid & use[:, None]
            xs.append(J), ys.append(torch.where(s_[..., None], T(prob.joints), zero)), ws.append(torch.where(s_, kj * cf, zero))
        if prob.verts is not None:
            w_root = M._tt(KIND, prob.side, dt)['weights'][:, 0]
            xs.append(V), ys.append(torch.where(use[:, None, None], T(prob.verts), zero)), ws.append(torch.where(use[:, None], (kv * w_root)[None], zero))
        x, y, w = torch.cat(xs, 1), torch.cat(ys, 1), torch.cat(ws, 1)
        xr, yr = x - pi[:, None], y - pi[:, None]
        S = torch.einsum('np,npa,npb->nab', w, xr, yr)
        e0 = (w * ((x - y) ** 2).sum(-1)).sum(1)
        W = w.sum(1)
        Q = horn_rotation(S)
        e1 = (w * ((torch.einsum('nab,npb->npa', Q, xr) + pi[:, None] - y) ** 2).sum(-1)).sum(1)
        acc = use & (W > 0) & (S != 0).reshape(n, 9).any(1) & (e1 <= e0)
        status = status | torch.where(use & ~acc, 8, 0)
        info[:, 0] = torch.where(use, e0, zero)
        info[:, 1] = torch.where(use, torch.where(acc, e1, e0), zero)
        R1 = torch.where(acc[:, None, None], Q @ R0, R1)
        Y = torch.where(acc[:, None, None], torch.einsum('nab,npb->npa', Q, J - pi[:, None]) + pi[:, None], J)
        new_root = acc
    # ---- steps 3 and 4
    cam0, camn = p[:, 61:64], p[:, 61:64].clone()
    choice = torch.full((n,), -1, dtype=torch.int64)
    e_k = torch.full((n, 24), float('inf'), dtype=dt)
    if prob.joint_uv is not None:
        s_, cf = sel['u']
        s_ = s_ & use[:, None]
        U, d = torch.where(s_[..., None], T(prob.joint_uv), zero), torch.where(s_, cf, zero)
        before = residual_uv(J[:, :, :2], U, d, cam0[:, 0], cam0[:, 1:3])
        after = residual_uv(Y[:, :, :2], U, d, cam0[:, 0], cam0[:, 1:3])
        if not have3d and root and cam and search:
            best, eb, fits = torch.full((n,), -1, dtype=torch.int64), torch.full((n,), float('inf'), dtype=dt), []
            for k, P in enumerate(cube_rotations()):
                Xk = torch.einsum('ab,npb->npa', torch.from_numpy(P).to(dt), J - pi[:, None]) + pi[:, None]
                s, t, e, den = camera_fit(Xk[:, :, :2], U, d)
                good = use & (den > 0) & torch.isfinite(s) & (s > 0) & torch.isfinite(e)
                fits.append((s, t))
                e_k[:, k] = torch.where(good, e, e_k[:, k])
                take = good & ((best < 0) | (e < eb))
                best, eb = torch.where(take, k, best), torch.where(take, e, eb)
            acc = use & (best >= 0) & (eb <= before)
            status = status | torch.where(use & ~acc, 8 | 16, 0)
            Ps = torch.from_numpy(cube_rotations()).to(dt)
            for i in range(n):
                if bool(acc[i]):
                    k = int(best[i])
                    R1[i] = Ps[k] @ R0[i]
                    camn[i, 0], camn[i, 1:3] = fits[k][0][i], fits[k][1][i]
                    choice[i] = k
            new_root = acc
            after = torch.where(acc, eb, before)
        elif cam:
            s, t, e, den = camera_fit(Y[:, :, :2], U, d)
            acc = use & (den > 0) & torch.isfinite(s) & (s > 0) & torch.isfinite(e) & (e <= after)
            status = status | torch.where(use & ~acc, 16, 0)
            camn = torch.where(acc[:, None], torch.cat([s[:, None], t], 1), camn)
            after = torch.where(acc, e, after)
        info[:, 2], info[:, 3] = torch.where(use, before, zero), torch.where(use, after, zero)
    para = p0.clone()
    para[:, 0:3] = torch.where(new_root[:, None], R1[:, :, 0], p0[:, 0:3])
    para[:, 3:6] = torch.where(new_root[:, None], R1[:, :, 1], p0[:, 3:6])
    para[:, 61:64] = torch.where(use[:, None], camn, p0[:, 61:64])
    return {'para': para, 'status': status, 'choice': choice, 'info': info, 'R1': R1, 'e_k': e_k}


# ===================================================================================================================== cases
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def far_truth(n, side, lo, hi, seed=0):
    """mano_fit_ref.truth's hands with the root a rotation by an angle in [lo, hi] rad about a random axis (orthonormal 6D columns)"""
    out = R.truth(n, side, seed)
    r = M._rng('start.truth.%s.%d' % (side, seed))
    for i in range(n):
        rot = rotation(r.normal(0, 1, 3), r.uniform(lo, hi))
        out[i, 0:3], out[i, 3:6] = rot[:, 0], rot[:, 1]
    return out


def root_of(para):
    """the float64 root rotation [n,3,3] of parameters (numpy or torch)"""
    with torch.no_grad():
        return M.robust_rot6d(torch.as_tensor(np.asarray(para), dtype=torch.float64)[:, :6])


def angle_between(Ra, Rb):
    """rotation angle of Ra^T Rb per row [n] (float64), by the chord: accurate at small angles"""
    d = (Ra.double() - Rb.double()).reshape(-1, 9).norm(dim=1)                 # |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2)
    return 2.0 * torch.asin((d / (2.0 * np.sqrt(2.0))).clamp(max=1.0))


def case(name, side, n=3, seed=0):
    """the canonical case `name` of CASE_NAMES -> (Problem, truth parameters [n,64] float32)"""
    lo, hi = (2.6, 3.14) if name in ('joints', 'uv') else (1.8, 3.1)
    center, root_palm = (-1 if name == 'centre-1' else R.CENTER), name == 'root_palm'
    p = far_truth(n, side, lo, hi, seed)
    t = R.targets_of(p, side, center, root_palm)
    r = M._rng('start.case.%s.%s.%d' % (name, side, seed))
    zero = dict.fromkeys(R.WEIGHTS, 0.0)
    cold = R.neutral_para(n, 4.0).numpy().astype(np.float32)
    verts = joints = jconf = uv = uconf = None
    w = dict(zero)
    if name in ('mesh', 'all', 'centre-1'):
        verts, w['w_verts'] = t['verts'], 1e4
    if name in ('joints', 'all', 'centre-1', 'root_palm'):
        joints, w['w_joints'] = t['joints'].copy(), 1e4
        jconf = r.uniform(0.2, 1.0, (n, 21)).astype(np.float32)
        if name == 'joints':
            jconf[:, [5, 11]] = 0.0
            joints[:, [5, 11]] = np.nan
    if name in ('all', 'uv', 'centre-1', 'root_palm'):
        uv, w['w_uv'] = t['joint_uv'].copy(), 1.0
        uconf = np.ones((n, 21), np.float32)
        if name == 'all':
            for i in range(n):
                j = int(r.randint(21))
                uconf[i, j] = 0.0
                uv[i, j] = np.nan
    lr = (0.03,) * 4 if name == 'uv' else (0.1,) * 4
    return R.Problem('%s_%s' % (name, side), side, center, root_palm, cold, verts, joints, jconf, uv, uconf, w, lr), p


def differences(got, ref):
    """{output: largest difference of `got` (dict with para, info; any dtype) from the float64 run `ref`} in the GATES' measures"""
    rel = (got['info'].double() - ref['info']).abs() / torch.where(ref['info'] != 0, ref['info'].abs(), torch.ones_like(ref['info']))
    return {'root': float(angle_between(root_of(got['para']), root_of(ref['para'])).max()),
            'cam': float((got['para'].double()[:, 61:64] - ref['para'][:, 61:64]).abs().max()), 'info': float(rel.max())}


def measure(name, n=3, sides=('right', 'left'), threads=(1, 4)):
    out = dict.fromkeys(OUTPUTS, 0.0)
    before = torch.get_num_threads()
    try:
        for nt in threads:
            torch.set_num_threads(nt)
            for side in sides:
                prob, _ = case(name, side, n)
                r32, r64 = start(prob, torch.float32), start(prob, torch.float64)
                assert r32['status'].tolist() == r64['status'].tolist() and r32['choice'].tolist() == r64['choice'].tolist(), (name, side)
                for k, v in differences(r32, r64).items():
                    out[k] = max(out[k], v)
    finally:
        torch.set_num_threads(before)
    return out


# Recorded from measure() on a CPU (float32 against float64 runs of THIS restatement; never the kernel).  tests/test_mano_start_ref.py re-measures every
# entry and fails where a re-measured figure exceeds its record.
GATES = {
    'mesh': {'root': 2.9e-07, 'cam': 0.0, 'info': 2.6e-07},
    'joints': {'root': 4.4e-07, 'cam': 0.0, 'info': 2.0e-06},
    'all': {'root': 5.8e-07, 'cam': 1.3e-06, 'info': 2.3e-06},
    'uv': {'root': 0.0, 'cam': 4.6e-07, 'info': 1.4e-07},
    'centre-1': {'root': 3.1e-07, 'cam': 2.2e-06, 'info': 1.1e-06},
    'root_palm': {'root': 2.4e-07, 'cam': 1.8e-06, 'info': 1.6e-06},
}


def gate(name, output):
    """the GPU test's bound on |kernel - float64 restatement|: MARGIN x the recorded float32-against-float64 difference"""
    return MARGIN * GATES[name][output]


# Recorded from tests/test_mano_start_ref.py's value test (float64, 4 rows; mesh right, joints left: the term's RMS in mm; 2-D left: the root's angle
# to the truth in rad): VALUE[case][iterations] = ((cold, started) at the best row, (cold, started) at the worst row).  Cold / started per row:
# mesh 8.2 .. 16.1 x at 50 iterations and 770 .. 10600 x at 200; joints 6.6 .. 12.1 x and 4.2 .. 19.9 x; 2-D 13 .. 150 x.
VALUE = {
    'mesh': {50: ((7.92, 0.969), (16.42, 1.032)), 200: ((0.353, 0.00037), (3.909, 0.00054))},
    'joints': {50: ((6.40, 0.677), (11.09, 1.674)), 200: ((1.09, 0.164), (5.09, 0.438))},
    'uv': {400: ((0.995, 0.0105), (1.567, 0.0746))},
}
