"""TEST INFRASTRUCTURE (CPU only: torch CPU): the rule of dir_mano_para_smooth_step (include/dir_hip.h, "smoothing in MANO parameter space")
restated in torch, parametrised by dtype (float64: the reference; float32: the kernel's precision), in the header's operation order.  The
forward from (R, aa, betas) is mano_cases' restatement (tables _tt, robust_rot6d, batch_rodrigues, the chain, fold=True order) entered behind the
PCA product; the finger, camera and history logic follows one_euro_ref.py.  One hand per object: the hands are independent.

    ref = ParaSmoothRef(side, batch, dt=torch.float64, center=9, root_palm=False, fps=30, ..., shape_frames=None)
    out = ref.step(para [B,64], cam_px [B,3], valid=None, raw=None)     # raw: dict verts [B,778,3], joints [B,21,3], joints_px [B,21,2] (any may miss)
    out: smoothed [B,64], verts, joints, joints_px (dtype dt), updated (int32 numpy);  ref.measures float64 [batch,8], ref.count, ref.n_shape, ...

Discrete decisions (finite, valid, the 1e-6 threshold rounded to the run's dtype) are taken on the run's own values.

RIGID BONES   with root_palm off, joints 0 and 1+4f, 2+4f, 3+4f of finger f are chain joints: their distances depend on the betas only.  The tip
joints 4+4f are skinned VERTICES: the tip bones (3+4f, 4+4f) bend with the pose and are not rigid.  RIGID lists the 15 rigid bones, BONES all 20.

CANONICAL CASE   parity_case(side): 3 sequences x 12 frames at fps 30, max_gap 4, shape_frames 3; root steps of 0.1 .. 0.3 rad per frame about a
fixed axis plus 0.02 rad of noise, PCA coefficients N(0, 0.4) with a slow drift (finger axis-angle norms stay below 2 rad: asserted by
tests/test_para_smooth_ref.py), betas that keep changing; sequence 0 has valid = 0 on frames 3 and 4, sequence 1 on frames 3 .. 7 (a gap beyond
max_gap), sequence 2 a NaN in the LEFT hand's betas on frame 5.  A reflection root is not in the case: for finite inputs the robust-6D
determinant is (x' x y') . normalise(x' x y') >= 0, and a search of 100 000 near-parallel float32 inputs found none below 0.

GATES   the largest |float32 run - float64 run| per output over parity_case, both sides, recorded here from a CPU run and re-measured by
tests/test_para_smooth_ref.py (which fails when a re-measured figure exceeds its record).  The GPU test allows MARGIN = 4 x the record.  Nothing
here is measured on the kernel.
"""
import math
import os
import sys

import numpy as np
import torch

_here = os.path.dirname(os.path.abspath(__file__))
if _here not in sys.path:
    sys.path.insert(0, _here)
import mano_cases as M  # noqa: E402
from oracle import mano as OM  # noqa: E402

KIND, CENTER = 'pca', 9
MARGIN = 4.0
BONES = tuple((0 if i == 0 else 4 * f + i, 4 * f + i + 1) for f in range(5) for i in range(4))
RIGID = tuple(b for k, b in enumerate(BONES) if k % 4 != 3)
MEASURES = ('mesh_raw', 'mesh_fil', 'joint_raw', 'joint_fil', 'px_raw', 'px_fil', 'flicker_raw', 'flicker_fil')
AGE_MAX = 1 << 30


def forward(side, center, root_palm, R, aa, betas, kind=KIND):
    """mano_cases.mano_outputs(fold=True) entered behind the PCA product: R [B,3,3], aa [B,45] (mean included), betas [B,10] -> verts, joints"""
    X = M._Plain
    dt = aa.dtype
    T = M._tt(kind, side, dt)
    B = aa.shape[0]
    rot_map = M.batch_rodrigues(aa.reshape(B * 15, 3)).reshape(B, 135)
    pose_map = rot_map - torch.eye(3, dtype=dt).reshape(9).repeat(15)
    v_shaped = X.dot('vck,bk->bvc', T['shapedirs'], betas) + T['vt']
    th_j = X.dot('jck,bk->bjc', T['j_shapedirs'], betas) + T['j_template']
    v_posed = v_shaped + X.dot('vck,bk->bvc', T['posedirs'], pose_map)
    rots = rot_map.reshape(B, 15, 3, 3)
    lr = [rots[:, [i - 1 for i in L]] for L in (OM.LEV1, OM.LEV2, OM.LEV3)]
    lj = [th_j[:, L] for L in (OM.LEV1, OM.LEV2, OM.LEV3)]
    R0 = R[:, None].expand(B, 5, 3, 3)
    t0 = th_j[:, 0][:, None].expand(B, 5, 3)
    R1, t1 = M._compose(R0, t0, lr[0], lj[0] - t0, X)
    R2, t2 = M._compose(R1, t1, lr[1], lj[1] - lj[0], X)
    R3, t3 = M._compose(R2, t2, lr[2], lj[2] - lj[1], X)
    Rs = torch.cat([R0[:, :1], R1, R2, R3], 1)[:, OM.REORDER_T]
    ts = torch.cat([t0[:, :1], t1, t2, t3], 1)[:, OM.REORDER_T]
    t2_ = ts - X.dot('bkij,bkj->bki', Rs, th_j)
    Tr = X.dot('bkij,vk->bvij', Rs, T['weights'])
    Tt = X.dot('bki,vk->bvi', t2_, T['weights'])
    verts = X.dot('bvij,bvj->bvi', Tr, v_posed) + Tt
    jtr = ts
    if root_palm:
        jtr = torch.cat([((verts[:, 95] + verts[:, 22]) / 2.0)[:, None], jtr[:, 1:]], 1)
    jtr = torch.cat([jtr, verts[:, OM.TIPS[side]]], 1)[:, OM.REORDER_J]
    if center >= 0:
        c = jtr[:, center][:, None]
        jtr, verts = jtr - c, verts - c
    return verts, jtr


def pose_aa(side, pca, kind=KIND):
    """a_x = hands_mean + pca . comps, [B,45] in pca's dtype"""
    T = M._tt(kind, side, pca.dtype)
    return T['mean'] + torch.einsum('bk,kj->bj', pca, T['comps'])


def _det(R):
    """the kernel's determinant of a [3,3] matrix with columns x, y, z"""
    x, y, z = R[:, 0], R[:, 1], R[:, 2]
    return x[0] * (y[1] * z[2] - z[1] * y[2]) - y[0] * (x[1] * z[2] - z[1] * x[2]) + z[0] * (x[1] * y[2] - y[1] * x[2])


def _mm(A, B):
    """[3,3] x [3,3] with every sum of three products as ((p0 + p1) + p2)"""
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def _step_rotation(v):
    """batch_rodrigues without its 1e-8 offset (the header's E): angle = |v|, the identity at 0 -> [3,3]"""
    angle = torch.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if float(angle) == 0.0:
        return torch.eye(3, dtype=v.dtype)
    half = angle * 0.5
    return M.quat2mat(torch.cat([torch.cos(half)[None], torch.sin(half) * (v / angle)])[None]).reshape(3, 3)


def bone_lengths(joints, bones=BONES):
    """[..., 21, 3] -> [..., len(bones)] in float64"""
    j = joints.double()
    return torch.stack([(j[..., c, :] - j[..., p, :]).pow(2).sum(-1).sqrt() for p, c in bones], -1)


class ParaSmoothRef(object):
    def __init__(self, side, batch, dt=torch.float64, center=CENTER, root_palm=False, kind=KIND, fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                 max_gap=None, shape_frames=None, rot_speed_scale=100.0, cam_speed_scale=1.0):
        self.side, self.center, self.root_palm, self.kind, self.dt = side, center, root_palm, kind, dt
        self.fps, self.min_cutoff, self.beta, self.d_cutoff = float(fps), float(min_cutoff), float(beta), float(d_cutoff)
        self.max_gap = int(round(self.fps)) if max_gap is None else int(max_gap)
        self.shape_frames = int(round(self.fps)) if shape_frames is None else int(shape_frames)
        self.rot_scale, self.cam_scale = float(rot_speed_scale), float(cam_speed_scale)
        B = int(batch)
        self.prev, self.vel = torch.zeros(B, 64, dtype=dt), torch.zeros(B, 64, dtype=dt)
        self.y1, self.y2, self.x1, self.x2 = (torch.zeros(B, 2439, dtype=dt) for _ in range(4))
        self.n_shape, self.age, self.run, self.count = (np.zeros(B, np.int64) for _ in range(4))
        self.measures = np.zeros((B, 8))

    def c(self, x):
        return torch.tensor(x, dtype=self.dt)

    def _alpha(self, r, fc):
        one = self.c(1.0)
        return one / (one + one / (r * fc))

    def _one_euro(self, x, y1, h, a_d, r, dtf, scale):
        """dir_one_euro_step's step 4 on points [n,D] -> (y, new h)"""
        dx = (x - y1) / dtf
        dh = h + a_d * (dx - h)
        v2 = torch.zeros(x.shape[0], dtype=self.dt)
        for k in range(x.shape[1]):
            v2 = v2 + dh[:, k] * dh[:, k]
        fc = self.c(self.min_cutoff) + self.c(self.beta) * (self.c(scale) * torch.sqrt(v2))
        al = self._alpha(r, fc)
        return y1 + al[:, None] * (x - y1), dh

    def _root(self, b, Rx, a_d, r, dtf):
        """step 4's root update of row b -> (six [6], R_y [3,3]) or None for a break; the speed estimate is updated"""
        Rp = M.robust_rot6d(self.prev[b:b + 1, :6])[0]
        D = _mm(Rp.t().contiguous(), Rx)
        half = self.c(0.5)
        s = half * torch.stack([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        cc = half * (((D[0, 0] + D[1, 1]) + D[2, 2]) - self.c(1.0))
        n = torch.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        small = bool(n <= self.c(1e-6))
        if small and bool(cc < 0):
            return None
        w = s if small else (torch.atan2(n, cc) / n) * s
        dh = self.vel[b, 0:3] + a_d * (w / dtf - self.vel[b, 0:3])
        self.vel[b, 0:3] = dh
        v2 = ((self.c(0.0) + dh[0] * dh[0]) + dh[1] * dh[1]) + dh[2] * dh[2]
        fc = self.c(self.min_cutoff) + self.c(self.beta) * (self.c(self.rot_scale) * torch.sqrt(v2))
        al = self._alpha(r, fc)
        E = _step_rotation(al * w)
        Rt = _mm(Rp, E)
        six = torch.cat([Rt[:, 0], Rt[:, 1]])
        return six, M.robust_rot6d(six[None])[0]

    def step(self, para, cam_px, valid=None, raw=None):
        def take(a):                                 # arrays are float32 data; a torch tensor is taken as it is (the float64 closed forms)
            return a.to(self.dt) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float32)).to(self.dt)
        para, cam_px = take(para), take(cam_px)
        raw = {} if raw is None else {k: take(v) for k, v in raw.items() if v is not None}
        B = para.shape[0]
        assert B <= self.age.shape[0]
        with torch.no_grad():
            Rx = M.robust_rot6d(para[:, :6])
            a_x = pose_aa(self.side, para[:, 6:51], self.kind)
            smoothed = torch.cat([para[:, :6], a_x, para[:, 51:61], cam_px], 1).clone()
            Ry = Rx.clone()
            updated = np.zeros(B, np.int32)
            for b in range(B):
                finite = bool(torch.isfinite(para[b, :61]).all()) and bool(torch.isfinite(cam_px[b]).all())
                usable = (valid is None or int(valid[b]) != 0) and finite and not bool(_det(Rx[b]) < 0)
                if not usable:
                    if self.age[b] > 0:
                        self.age[b] = min(self.age[b] + 1, AGE_MAX)
                    self.run[b] = 0
                    continue
                mode = 2 if self.age[b] == 0 or self.age[b] > self.max_gap else 1
                if mode == 1:
                    dtd = self.age[b] / self.fps
                    dtf, r = self.c(dtd), self.c(2.0 * math.pi * dtd)
                    a_d = self.c(1.0 / (1.0 + 1.0 / (2.0 * math.pi * self.d_cutoff * dtd)))
                    root = self._root(b, Rx[b], a_d, r, dtf)
                    if root is None:
                        mode = 2
                    else:
                        smoothed[b, :6], Ry[b] = root
                        y, h = self._one_euro(a_x[b].reshape(15, 3), self.prev[b, 6:51].reshape(15, 3), self.vel[b, 6:51].reshape(15, 3), a_d, r, dtf, self.rot_scale)
                        smoothed[b, 6:51], self.vel[b, 6:51] = y.reshape(45), h.reshape(45)
                        y, h = self._one_euro(cam_px[b].reshape(3, 1), self.prev[b, 61:64].reshape(3, 1), self.vel[b, 61:64].reshape(3, 1), a_d, r, dtf, self.cam_scale)
                        smoothed[b, 61:64], self.vel[b, 61:64] = y.reshape(3), h.reshape(3)
                        self.run[b] = min(self.run[b] + 1, AGE_MAX)
                if mode == 2:
                    self.vel[b] = 0
                    self.run[b] = 1
                if self.shape_frames > 0:
                    mean = self.prev[b, 51:61].clone()
                    if self.n_shape[b] < self.shape_frames:
                        self.n_shape[b] += 1
                        n1 = int(self.n_shape[b])
                        mean = para[b, 51:61].clone() if n1 == 1 else mean + (para[b, 51:61] - mean) / self.c(float(n1))
                    smoothed[b, 51:61] = mean
                    self.prev[b, 51:61] = mean
                self.prev[b, :51], self.prev[b, 61:] = smoothed[b, :51], smoothed[b, 61:]
                self.age[b] = 1
                updated[b] = mode
            verts, joints = forward(self.side, self.center, self.root_palm, Ry, smoothed[:, 6:51], smoothed[:, 51:61], self.kind)
            px = smoothed[:, 61:62, None] * joints[:, :, :2] + smoothed[:, None, 62:64]
            y = torch.cat([verts.reshape(B, -1), joints.reshape(B, -1), px.reshape(B, -1)], 1)
            segs = ((0, 778, 3, 'verts'), (2334, 21, 3, 'joints'), (2397, 21, 2, 'joints_px'))
            for b in range(B):
                if updated[b] == 0:
                    continue
                if self.run[b] >= 3:
                    for s, (at, n, d, name) in enumerate(segs):
                        sl = slice(at, at + n * d)
                        df = y[b, sl].double() - 2 * self.y1[b, sl].double() + self.y2[b, sl].double()
                        self.measures[b, 2 * s + 1] += float(df.reshape(n, d).pow(2).sum(1).sqrt().sum())
                        if name in raw:
                            dr = raw[name][b].reshape(-1).double() - 2 * self.x1[b, sl].double() + self.x2[b, sl].double()
                            self.measures[b, 2 * s] += float(dr.reshape(n, d).pow(2).sum(1).sqrt().sum())
                    jl = slice(2334, 2397)
                    self.measures[b, 7] += float((bone_lengths(joints[b]) - bone_lengths(self.y1[b, jl].reshape(21, 3))).abs().sum())
                    if 'joints' in raw:
                        self.measures[b, 6] += float((bone_lengths(raw['joints'][b]) - bone_lengths(self.x1[b, jl].reshape(21, 3))).abs().sum())
                    self.count[b] += 1
                self.y2[b], self.y1[b] = self.y1[b].clone(), y[b].clone()
                for at, n, d, name in segs:
                    if name in raw:
                        sl = slice(at, at + n * d)
                        self.x2[b, sl] = self.x1[b, sl].clone()
                        self.x1[b, sl] = raw[name][b].reshape(-1)
        return {'smoothed': smoothed, 'verts': verts, 'joints': joints, 'joints_px': px, 'updated': updated}


# ===================================================================================================================== the canonical case
FRAMES, SEQS = 12, 3
CASE_OPTS = dict(fps=30.0, max_gap=4, shape_frames=3)


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def parity_case(side):
    """-> list of FRAMES dicts: para [3,64], cam_px [3,3] float32, valid int32 [3], raw = dict of float32 verts, joints, joints_px (the forward
    at the frame's own parameters, as the network's stage gives them; a non-finite row stays non-finite)"""
    r = M._rng('para_smooth.case.' + side)
    base_R = [_rot(r.normal(0, 1, 3), r.uniform(0, 1.0)) for _ in range(SEQS)]
    axis = [r.normal(0, 1, 3) for _ in range(SEQS)]
    step = [r.uniform(0.1, 0.3) for _ in range(SEQS)]
    pca0, pca1 = r.normal(0, 0.4, (SEQS, 45)), r.normal(0, 0.1, (SEQS, 45))
    beta0 = r.normal(0, 0.5, (SEQS, 10))
    cam0 = np.stack([r.uniform(150, 250, SEQS), r.uniform(200, 400, SEQS), r.uniform(200, 400, SEQS)], 1)
    frames = []
    for t in range(FRAMES):
        para = np.zeros((SEQS, 64), np.float32)
        cam = np.zeros((SEQS, 3), np.float32)
        for q in range(SEQS):
            R = base_R[q] @ _rot(axis[q], step[q] * t) @ _rot(r.normal(0, 1, 3), r.normal(0, 0.02))
            para[q, 0:3], para[q, 3:6] = R[:, 0] * r.uniform(0.7, 1.4), R[:, 1] * r.uniform(0.7, 1.4)
            para[q, 6:51] = pca0[q] + pca1[q] * np.sin(0.4 * t) + r.normal(0, 0.02, 45)
            para[q, 51:61] = beta0[q] + r.normal(0, 0.05, 10)
            para[q, 61:64] = r.normal(0, 1, 3)                      # the crop camera: not read
            cam[q] = cam0[q] + np.array([0.5 * t, 2.0 * t, -1.5 * t]) + r.normal(0, 0.5, 3)
        valid = np.ones(SEQS, np.int32)
        if t in (3, 4):
            valid[0] = 0
        if 3 <= t <= 7:
            valid[1] = 0
        if t == 5 and side == 'left':
            para[2, 55] = np.nan
        with torch.no_grad():
            p = torch.from_numpy(para.astype(np.float64))
            v, j = forward(side, CENTER, False, M.robust_rot6d(p[:, :6]), pose_aa(side, p[:, 6:51]), p[:, 51:61])
            c = torch.from_numpy(cam.astype(np.float64))
            px = c[:, 0:1, None] * j[:, :, :2] + c[:, None, 1:3]
        raw = {'verts': v.numpy().astype(np.float32), 'joints': j.numpy().astype(np.float32), 'joints_px': px.numpy().astype(np.float32)}
        frames.append({'para': para, 'cam_px': cam, 'valid': valid, 'raw': raw})
    return frames


def run_case(side, dt, frames=None, **opts):
    """the canonical case through ParaSmoothRef -> (list of per-frame outputs, ref)"""
    frames = parity_case(side) if frames is None else frames
    ref = ParaSmoothRef(side, SEQS, dt=dt, **dict(CASE_OPTS, **opts))
    return [ref.step(f['para'], f['cam_px'], f['valid'], f['raw']) for f in frames], ref


GROUPS = {'six': slice(0, 6), 'aa': slice(6, 51), 'betas': slice(51, 61), 'cam': slice(61, 64)}
OUTPUTS = ('six', 'aa', 'betas', 'cam', 'verts', 'joints', 'joints_px', 'jitter_rel', 'flicker_rel')


def _maxdiff(a, b):
    d = (a.double() - b.double()).abs()
    d = d[torch.isfinite(d)]
    return float(d.max()) if d.numel() else 0.0


def rel_measures(got, want):
    """largest |got - want| / want over the jitter sums (columns 0:6) and over the flicker sums (6:8), where want > 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(want > 0, np.abs(got - want) / want, 0.0)
    return float(rel[:, :6].max()), float(rel[:, 6:].max())


def measure(sides=('right', 'left'), threads=(1, 4)):
    """{output: largest |float32 run - float64 run|} of the restatement over parity_case, both sides (the larger over the thread counts, as
    mano_fit_ref.measure)"""
    out = dict.fromkeys(OUTPUTS, 0.0)
    before = torch.get_num_threads()
    try:
        for nt in threads:
            torch.set_num_threads(nt)
            for side in sides:
                frames = parity_case(side)
                (o32, r32), (o64, r64) = run_case(side, torch.float32, frames), run_case(side, torch.float64, frames)
                assert all((a['updated'] == b['updated']).all() for a, b in zip(o32, o64))
                for a, b in zip(o32, o64):
                    for g, sl in GROUPS.items():
                        out[g] = max(out[g], _maxdiff(a['smoothed'][:, sl], b['smoothed'][:, sl]))
                    for k in ('verts', 'joints', 'joints_px'):
                        out[k] = max(out[k], _maxdiff(a[k], b[k]))
                j, f = rel_measures(r32.measures, r64.measures)
                out['jitter_rel'], out['flicker_rel'] = max(out['jitter_rel'], j), max(out['flicker_rel'], f)
    finally:
        torch.set_num_threads(before)
    return out


# Recorded from measure() on a CPU (float32 against float64 runs of THIS restatement; never the kernel).  tests/test_para_smooth_ref.py re-measures
# every entry and fails where a re-measured figure exceeds its record.
GATES = {'six': 1.76e-07, 'aa': 3.02e-07, 'betas': 7.95e-08, 'cam': 1.81e-05, 'verts': 3.51e-08, 'joints': 2.24e-08, 'joints_px': 3.25e-05,
         'jitter_rel': 1.83e-05, 'flicker_rel': 1.05e-05}


def gate(output):
    """the GPU test's bound on |kernel - float64 restatement|: MARGIN x the recorded float32-against-float64 difference"""
    return MARGIN * GATES[output]
