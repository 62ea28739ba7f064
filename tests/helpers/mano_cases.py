"""TEST INFRASTRUCTURE (CPU only: numpy + torch CPU): the per-element gate of the MANO kernels -- dir_mano_forward / dir_mano_forward_pair
(csrc/mano.hip), dir_mano_backward_pair (csrc/mano_bwd.hip) and dir_gt_mano_forward (csrc/gtmano.hip).

check(got, ref, S, c)      every element: |got - ref| <= c 2^-24 S + floor, floor = half an ulp of the fp32 output + 2^-140.

TABLES   'pca'   synth.mano_buffers(side, SEED)
         'ident' the same with th_selected_comps = I and th_hands_mean = 0: the 45 pose inputs ARE the axis-angles, exactly (through the
                 synthetic PCA basis `hands_mean + pca @ comps` rounds at about 1e-8 rad, so an axis-angle of 1e-9 is unreachable).

RESTATEMENT   mano_outputs() follows oracle/mano.py line for line (||aa + 1e-8||, the quaternion re-normalisation, the clamp as
torch.maximum) and gt_outputs() follows oracle/gt_mano.py (classic Rodrigues with |axis| + 1e-8); both are torch, parametrised by dtype,
and run on plain tensors (float32 / float64, with autograd: float64 autograd is the backward reference) or on V = (value, running error
bound).  `fold=True` is the kernels' documented order where it differs from the oracle's: the joint regressor folded into j_template /
j_shapedirs (fp64 at pack time), and in the ground-truth layer t = j - R j instead of (I - R) j.

ERROR SCALE OF THE FORWARD: a running bound e carried next to every float64 value, u = 2^-24; S = e(out) / u, the larger of the two orders.
    inputs and tables       e = 0 (they are fp32 numbers); the constants 1e-8: e = u 1e-8 (fp32 cannot hold 1e-8)
    c = a + b, a - b        e(c) = e(a) + e(b) + u |c|
    c = a b                 e(c) = |b| e(a) + |a| e(b) + u |c|
    c = a / b               e(c) = e(a) / |b| + |a| e(b) / b^2 + u |c|
    c = sqrt(a)             e(c) = e(a) / (2 sqrt(a)) + u |c|
    sin(x), cos(x)          |cos x| e(x) + 2u resp. |sin x| e(x) + 2u  (fp32 sinf / cosf: within 2 units of 2^-24, absolute)
    max(a, 1e-8)            e(a) + u 1e-8 (the clamp passes e through)
    sum of n products       sum (|a| e(b) + e(a) |b|) + n u sum |a| |b|; n = the number of non-zero products (4 skinning weights, 24
                            regressor entries per row)
  stage by stage: PCA (n = 45) -> + 1e-8, norm (n = 3), division, half, cos / sin, quaternion norm (n = 4), the 9 quadratic forms ->
  R - I -> the seven normalisations of the robust 6D root (every one divides e by |v|: S grows like 1 / |x^ - y^| for near-parallel and
  like 1 / |x^ + y^| for anti-parallel columns, and like the angle through cos / sin: that is the point of using it) -> shape blend
  (n = 10), joint regression (n = 24 or 10), pose blend (n = 135) -> three chain levels (n = 3 and 4) -> A' = A - A.J -> skinning (n = 4,
  then n = 4) -> tips, reorder, centre -> s xy + t.

ERROR SCALE OF THE BACKWARD   S_k = sum_i |J_ik| |cot_i| + |g_k|, J the float64 Jacobian of the four outputs (forward-mode autograd, 64
tangents), kept per column group: root 0:6, PCA 6:51, betas 51:61, cam scale 61, cam translation 62:64.

CONSTANTS  c is NOT measured on the kernels: c = 4 x the largest |ref32 - ref64| / (2^-24 S) over the list, ref32 = the worse of (a) the
numpy oracle in float32 and (b) the restatement in float32 in the kernels' order (forward), resp. of torch float32 autograd through the
restatement (both orders, one thread) and tests/golden/g13_mano_grad.npz (backward, per (column group, root class, joint class)).  4 = the project's margin for
another valid order.  RATIOS records every reference ratio; tests/test_mano_cases_ref.py re-measures them.

GATES OF THE ROOT   loose: the 6D input is the operand, S carries the conditioning of the seven normalisations.  tight ('root as
operand'): the float64 reference takes the 3x3 root from the float32 numpy robust_rot6d (the kernel promises that op sequence, no FMA
contraction) and S is that of an exact root -- the tight gate for near_parallel / anti_parallel / sub_clamp.

DEGENERATE   exactly parallel columns, a zero column, both zero, and every near / anti-parallel eps at which the loose tolerance
exceeds 2^-8 of the sample's max |verts|: held only to finite outputs, the flag of the float32 restatement, guards and bit-equal repeats.

defects()   single defects of the restatement that check() must reject somewhere in the list; OLD_GATES_ACCEPT names those that the
max-norm gates that preceded this file (1e-7 m on positions, 2e-6 on projections, 1e-5 of the gradient's maximum over [B, 64]), applied to
the benign cases of this list, accept (OLD_SUITE_BLIND: one more that the old suite's own root_palm test could not see).
"""
import collections
import functools
import zlib

import numpy as np
import torch

from dir_amd import synth
from oracle import mano as OM

SEED = 1234
U = 2.0 ** -24
TINY = 2.0 ** -140
KINDS = ('verts', 'joints', 'joint_uv', 'mesh_uv')
GROUPS = collections.OrderedDict([('root', slice(0, 6)), ('pca', slice(6, 51)), ('betas', slice(51, 61)), ('cam_s', slice(61, 62)), ('cam_t', slice(62, 64))])
PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
GT_TIPS = (745, 317, 444, 556, 673)
TIP_CENTRES = (4, 12, 20)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


# ===================================================================================================================== tables
@functools.lru_cache(maxsize=None)
def tables(kind, side):
    """the th_* buffers (float32 numpy) of table set `kind` in ('pca', 'ident')"""
    buf = dict(synth.mano_buffers(side, SEED))
    if kind == 'ident':
        buf['th_selected_comps'] = np.eye(45, dtype=np.float32)
        buf['th_comps'] = np.eye(45, dtype=np.float32)
        buf['th_hands_mean'] = np.zeros((1, 45), np.float32)
    return buf


def state_dict(kind, side, prefix='m'):
    """what engine.pack_mano takes (CPU tensors; the GPU test moves them)"""
    return {prefix + '.' + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tables(kind, side).items()}


@functools.lru_cache(maxsize=None)
def _tt(kind, side, dt):
    b = tables(kind, side)
    t64 = {k: torch.from_numpy(np.asarray(b[k], np.float64)) for k in ('th_shapedirs', 'th_posedirs', 'th_v_template', 'th_J_regressor', 'th_weights',
                                                                       'th_hands_mean', 'th_selected_comps')}
    T = dict(comps=t64['th_selected_comps'], mean=t64['th_hands_mean'].reshape(45), shapedirs=t64['th_shapedirs'], posedirs=t64['th_posedirs'],
             vt=t64['th_v_template'].reshape(778, 3), jreg=t64['th_J_regressor'], weights=t64['th_weights'])
    # the fold of engine.pack_mano: fp64 products rounded to fp32
    T['j_template'] = (T['jreg'] @ T['vt']).float().double()
    T['j_shapedirs'] = torch.einsum('jv,vck->jck', T['jreg'], T['shapedirs']).float().double()
    return {k: v.to(dt) for k, v in T.items()}


# ===================================================================================================================== values with a running bound
class V(object):
    """float64 value v with the running bound e of its fp32 evaluation (module docstring)"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def of(a):
        return a if isinstance(a, V) else V(torch.as_tensor(a, dtype=torch.float64))

    shape = property(lambda s: s.v.shape)

    def __add__(a, b):
        b = V.of(b); v = a.v + b.v
        return V(v, a.e + b.e + U * v.abs())
    __radd__ = __add__

    def __sub__(a, b):
        b = V.of(b); v = a.v - b.v
        return V(v, a.e + b.e + U * v.abs())

    def __rsub__(a, b):
        return V.of(b) - a

    def __mul__(a, b):
        b = V.of(b); v = a.v * b.v
        return V(v, a.e * b.v.abs() + a.v.abs() * b.e + U * v.abs())
    __rmul__ = __mul__

    def __truediv__(a, b):
        b = V.of(b); v = a.v / b.v
        return V(v, a.e / b.v.abs() + a.v.abs() * b.e / (b.v * b.v) + U * v.abs())

    def __neg__(a):
        return V(-a.v, a.e)

    def __getitem__(a, i):
        return V(a.v[i], a.e[i])

    def reshape(a, *shape):
        return V(a.v.reshape(*shape), a.e.reshape(*shape))


class _Plain(object):
    """the operations of the restatement on plain tensors"""
    sqrt, sin, cos, cat, stack = torch.sqrt, torch.sin, torch.cos, torch.cat, torch.stack

    @staticmethod
    def const(c):
        return c

    @staticmethod
    def maxc(a, c):
        return torch.maximum(a, torch.tensor(c, dtype=a.dtype))

    @staticmethod
    def dot(spec, a, b, n=None):
        return torch.einsum(spec, a, b)

    @staticmethod
    def sum(a, dim):
        return a.sum(dim, keepdim=True)

    @staticmethod
    def map(a, f):
        return f(a)


class _Bound(object):
    """the same operations on V"""
    @staticmethod
    def sqrt(a):
        v = torch.sqrt(a.v)
        return V(v, torch.where(v > 0, a.e / (2 * v), torch.sqrt(a.e)) + U * v)

    @staticmethod
    def sin(a):
        return V(torch.sin(a.v), torch.cos(a.v).abs() * a.e + 2 * U)

    @staticmethod
    def cos(a):
        return V(torch.cos(a.v), torch.sin(a.v).abs() * a.e + 2 * U)

    @staticmethod
    def const(c):
        return V(torch.tensor(c, dtype=torch.float64), torch.tensor(U * abs(c), dtype=torch.float64))

    @staticmethod
    def maxc(a, c):
        return V(torch.clamp_min(a.v, c), a.e + U * c)

    @staticmethod
    def dot(spec, a, b, n=None):
        a, b = V.of(a), V.of(b)
        if n is None:
            ins, out = spec.split('->')
            ia, ib = ins.split(',')
            n = 1
            for ch, d in zip(ia, a.v.shape):
                if ch in ib and ch not in out:
                    n *= d
        aa, ab = a.v.abs(), b.v.abs()
        e = n * U * torch.einsum(spec, aa, ab)
        if bool((b.e != 0).any()):
            e = e + torch.einsum(spec, aa, b.e)
        if bool((a.e != 0).any()):
            e = e + torch.einsum(spec, a.e, ab)
        return V(torch.einsum(spec, a.v, b.v), e)

    @staticmethod
    def sum(a, dim):
        return V(a.v.sum(dim, keepdim=True), a.e.sum(dim, keepdim=True) + a.v.shape[dim] * U * a.v.abs().sum(dim, keepdim=True))

    @staticmethod
    def cat(xs, dim):
        xs = [V.of(x) for x in xs]
        return V(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim))

    @staticmethod
    def stack(xs, dim):
        xs = [V.of(x) for x in xs]
        return V(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))

    @staticmethod
    def map(a, f):
        return V(f(a.v), f(a.e))


def _ops(x):
    return _Bound if isinstance(x, V) else _Plain


def _fake_grad(value, v, dv):
    """`value` with the gradient d value / d v = dv imposed (the backward defects: a wrong chain-rule factor at an unchanged forward)"""
    lin = (v * dv.detach()).sum(-1, keepdim=True)
    return value.detach() + lin - lin.detach()


# ===================================================================================================================== the network's MANO layer
def normalize_vector(v, mut=None):
    """rot6d.py:54-60: v / max(||v||, 1e-8)"""
    X = _ops(v)
    raw = X.sqrt(X.sum(v * v, 1))
    mag = X.maxc(raw, 1e-8)
    if mut == 'bwd_clamp_projects' and X is _Plain:
        # mano_bwd.hip before the fix: (g - n (n.g)) / mag with mag = 1e-8 in the clamped branch too, i.e. d mag / d v = v / mag there
        mag = torch.where(raw < 1e-8, _fake_grad(mag, v, v / mag), mag)
    return v / mag


def _cross(u, v):
    X = _ops(u)
    return X.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def robust_rot6d(p6, mut=None):
    """rot6d.py:26-51, columns (x', y', z)"""
    X = _ops(p6)
    x = normalize_vector(p6[:, 0:3], mut)
    y = normalize_vector(p6[:, 3:6], mut)
    middle = normalize_vector(x + y, mut)
    orthmid = normalize_vector(x - y, mut)
    x = normalize_vector(middle + orthmid, mut)
    y = normalize_vector(middle - orthmid, mut)
    z = normalize_vector(_cross(x, y), mut)
    return X.stack([x, y, z], 2)


def quat2mat(q, renorm=True):
    """rodrigues_layer.py:15-40"""
    X = _ops(q)
    if renorm:
        q = q / X.sqrt(X.sum(q * q, 1))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz = w * x, w * y, w * z
    xy, xz, yz = x * y, x * z, y * z
    return X.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                    2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                    2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1)


def batch_rodrigues(aa, mut=None):
    """rodrigues_layer.py:43-54: angle = ||aa + 1e-8||, axis = aa / angle, quaternion (cos(a/2), sin(a/2) axis) -> quat2mat.  [N,3] -> [N,9]"""
    X = _ops(aa)
    if mut == 'angle_eps_outside':
        angle = X.sqrt(X.sum(aa * aa, 1)) + X.const(1e-8)
    else:
        ex = aa + X.const(1e-8)
        angle = X.sqrt(X.sum(ex * ex, 1))
        if mut == 'bwd_angle_without_eps':
            angle = _fake_grad(angle, aa, aa / angle)
    axis = aa / angle
    half = angle * 0.5
    quat = X.cat([X.cos(half), X.sin(half) * axis], 1)
    return quat2mat(quat, renorm=mut != 'no_quat_renorm')


def _compose(Ra, ta, Rb, tb, X):
    """[Ra | ta] . [Rb | tb] over the leading dimensions [B, F]"""
    return X.dot('bfij,bfjk->bfik', Ra, Rb), X.dot('bfij,bfj->bfi', Ra, tb) + ta


def mano_outputs(kind, side, center, para, root_palm=False, root_mat=None, fold=False, mut=None):
    """the four tensors a stage derives from a hand's 64-vector: verts [B,778,3], joints [B,21,3], joint_uv [B,21,2], mesh_uv [B,778,2].
    para: [B,64] tensor (float32 / float64) or V.  root_mat [B,3,3]: the root rotation as an operand instead of para[:, :6]."""
    X = _ops(para)
    dt = torch.float64 if X is _Bound else para.dtype
    T = _tt(kind, side, dt)
    B = para.shape[0]
    pose, betas, cam = para[:, :51], para[:, 51:61], para[:, 61:64]
    full = T['mean'] + X.dot('bk,kj->bj', pose[:, 6:51], T['comps'])                                  # manolayer.py:136-144
    rot_map = X.map(batch_rodrigues(X.map(full, lambda t: t.reshape(B * 15, 3)), mut), lambda t: t.reshape(B, 135))     # :153
    eye = torch.eye(3, dtype=dt).reshape(9).repeat(15)
    pose_map = rot_map - eye if mut != 'pose_map_is_R' else rot_map + 0.0 * eye                       # tensutils.py:34-42
    root_rot = robust_rot6d(pose[:, :6], mut) if root_mat is None else root_mat                       # :155
    v_shaped = X.dot('vck,bk->bvc', T['shapedirs'], betas) + T['vt']                                  # :180-182
    jbetas = betas.detach() if mut == 'bwd_betas_without_joints' else betas
    if fold:
        th_j = X.dot('jck,bk->bjc', T['j_shapedirs'], jbetas) + T['j_template']
    elif mut == 'bwd_betas_without_joints':
        th_j = X.dot('jv,bvc->bjc', T['jreg'], X.dot('vck,bk->bvc', T['shapedirs'], jbetas) + T['vt'], n=24)
    else:
        th_j = X.dot('jv,bvc->bjc', T['jreg'], v_shaped, n=24)                                        # :183
    pm = pose_map.detach() if mut == 'bwd_no_pose_blend' else pose_map
    v_posed = v_shaped + X.dot('vck,bk->bvc', T['posedirs'], pm)                                      # :186-187
    rots = X.map(rot_map, lambda t: t.reshape(B, 15, 3, 3))
    lr = [rots[:, [i - 1 for i in L]] for L in (OM.LEV1, OM.LEV2, OM.LEV3)]
    lj = [th_j[:, L] for L in (OM.LEV1, OM.LEV2, OM.LEV3)]
    R0 = X.map(root_rot, lambda t: t[:, None].expand(B, 5, 3, 3))
    t0 = X.map(th_j[:, 0], lambda t: t[:, None].expand(B, 5, 3))
    R1, t1 = _compose(R0, t0, lr[0], lj[0] - t0, X)                                                   # :210-214
    Rp, tp = R1, t1
    if mut == 'level2_parent_of_neighbour':
        Rp, tp = (X.map(a, lambda t: torch.roll(t, 1, 1)) for a in (R1, t1))
    R2, t2 = _compose(Rp, tp, lr[1], lj[1] - lj[0], X)                                                # :217-220
    Rp, tp = (R2.detach(), t2.detach()) if mut == 'bwd_no_chain_carry' else (R2, t2)
    R3, t3 = _compose(Rp, tp, lr[2], lj[2] - lj[1], X)                                                # :223-226
    Rs = X.cat([R0[:, :1], R1, R2, R3], 1)[:, OM.REORDER_T]                                           # :228-229   [B,16,3,3]
    ts = X.cat([t0[:, :1], t1, t2, t3], 1)[:, OM.REORDER_T]
    t2_ = ts - X.dot('bkij,bkj->bki', Rs, th_j)                                                       # :232-234
    Tr = X.dot('bkij,vk->bvij', Rs, T['weights'], n=4)                                                # :236
    Tt = X.dot('bki,vk->bvi', t2_, T['weights'], n=4)
    verts = X.dot('bvij,bvj->bvi', Tr, v_posed) + Tt                                                  # :245-246
    if mut == 'vertex_196_unskinned':
        verts = X.cat([verts[:, :196], v_posed[:, 196:197], verts[:, 197:]], 1)
    jtr = ts                                                                                          # :247
    if root_palm:
        palm = (verts[:, 95] + verts[:, 21 if mut == 'root_palm_vertex_21' else 22]) / 2.0
        jtr = X.cat([palm[:, None], jtr[:, 1:]], 1)
    tip_ids = OM.TIPS['right' if mut == 'left_tip_444' else side]
    tips = verts[:, tip_ids]
    if mut == 'bwd_tip_cotangent_dropped':
        tips = tips.detach()
    jtr = X.cat([jtr, tips], 1)[:, OM.REORDER_J]                                                      # :249-259
    if center >= 0:                                                                                   # :261-265
        c = jtr[:, (center + 1) % 21 if mut == 'centre_on_next_joint' else center][:, None]
        if mut == 'bwd_centre_sum_dropped':
            c = c.detach()
        jtr, verts = jtr - c, verts - c
    s, t = cam[:, 0][:, None, None], cam[:, 1:3][:, None]                                             # utils/utils.py:47-63
    if mut == 'ty_used_for_u':
        t = cam[:, [2, 2]][:, None]
    sj = s.detach() if mut == 'bwd_cam_s_without_joint_uv' else s
    return verts, jtr, sj * jtr[:, :, :2] + t, s * verts[:, :, :2] + t


# ===================================================================================================================== the ground-truth layer
def rodrigues_classic(axis):
    """models/manolayer.py:32-48: [n,3] -> [n,3,3]"""
    X = _ops(axis)
    angle = X.sqrt(X.sum(axis * axis, 1)) + X.const(1e-8)
    axes = axis / angle
    sin, cos = X.sin(angle)[:, :, None], X.cos(angle)[:, :, None]
    z = axes[:, 0] * 0.0
    L = X.stack([X.stack([z, -axes[:, 2], axes[:, 1]], 1), X.stack([axes[:, 2], z, -axes[:, 0]], 1), X.stack([-axes[:, 1], axes[:, 0], z], 1)], 1)
    dt = torch.float64 if X is _Bound else axis.dtype
    return torch.eye(3, dtype=dt)[None] + sin * L + (1.0 - cos) * X.dot('nij,njk->nik', L, L)


def gt_outputs(kind, side, root, pose, shape, ncomps=45, center=-1, scale=None, trans=None, new_skel=False, fold=False, mut=None):
    """models/manolayer.py:251-323 as oracle/gt_mano.py restates it.  root [B,3,3]; pose [B,ncomps] or, with ncomps = 0, [B,15,3,3]."""
    X = _ops(shape)
    dt = torch.float64 if X is _Bound else shape.dtype
    T = _tt(kind, side, dt)
    B = shape.shape[0]
    eye = torch.eye(3, dtype=dt)
    if ncomps > 0:
        axis = X.dot('bk,kj->bj', pose, T['comps'][:ncomps]) + T['mean']                              # :161-174
        rot = X.map(rodrigues_classic(X.map(axis, lambda t: t.reshape(B * 15, 3))), lambda t: t.reshape(B, 15, 3, 3))
    else:
        rot = pose
    v_shaped = T['vt'] + X.dot('vck,bk->bvc', T['shapedirs'], shape)                                  # :265-266
    j_tpose = X.dot('jck,bk->bjc', T['j_shapedirs'], shape) + T['j_template'] if fold else X.dot('jv,bvc->bjc', T['jreg'], v_shaped, n=24)
    pose_shape = X.map(rot, lambda t: t.reshape(B, 135)) - eye.reshape(9).repeat(15)                  # :270-271
    v_tpose = v_shaped + X.dot('vck,bk->bvc', T['posedirs'], pose_shape)                              # :272-273

    def local(R, j):
        return (j - X.dot('bij,bj->bi', R, j)) if fold else X.dot('bij,bj->bi', eye - R, j)

    Rs, ts = [root], [local(root, j_tpose[:, 0])]                                                     # :275-278
    for i in range(1, 16):                                                                            # :279-283
        R, p = rot[:, i - 1], PARENT[i]
        Rs.append(X.dot('bij,bjk->bik', Rs[p], R))
        ts.append(X.dot('bij,bj->bi', Rs[p], local(R, j_tpose[:, i])) + ts[p])
    jl = [j_tpose[:, 0]] + [X.dot('bij,bj->bi', Rs[PARENT[i]], j_tpose[:, i]) + ts[PARENT[i]] for i in range(1, 16)]    # :286-289
    Rs, ts = X.stack(Rs, 1), X.stack(ts, 1)
    Tr = X.dot('bkij,vk->bvij', Rs, T['weights'], n=4)                                                # :292
    Tt = X.dot('bki,vk->bvi', ts, T['weights'], n=4)
    v_out = X.dot('bvij,bvj->bvi', Tr, v_tpose) + Tt                                                  # :294-295
    tips = [745, 317, 445, 556, 673] if (mut == 'gt_left_tip_445' and side == 'left') else list(GT_TIPS)
    j_out = X.cat([X.stack(jl, 1), v_out[:, tips]], 1)[:, OM.REORDER_J]                               # :297-300
    if mut == 'gt_scale_before_centre':
        sc = scale.reshape(B, 1, 1) if scale is not None else 1.0
        c = j_out[:, center:center + 1] if center >= 0 else 0.0
        v_out, j_out = v_out * sc - c, j_out * sc - c
    else:
        if center >= 0:                                                                               # :302-305
            c = j_out[:, center:center + 1]
            v_out, j_out = v_out - c, j_out - c
        if scale is not None:                                                                         # :307-310
            v_out, j_out = v_out * scale.reshape(B, 1, 1), j_out * scale.reshape(B, 1, 1)
    if trans is not None:                                                                             # :312-315
        v_out, j_out = v_out + trans.reshape(B, 1, 3), j_out + trans.reshape(B, 1, 3)
    if new_skel:                                                                                      # :317-321
        pairs = {5: (63, 144), 9: (271, 221) if mut == 'gt_new_skel_wrong_pair' else (271, 220), 13: (148, 290), 17: (770, 83)}
        j_out = X.cat([((v_out[:, pairs[j][0]] + v_out[:, pairs[j][1]]) / 2.0)[:, None] if j in pairs else j_out[:, j:j + 1] for j in range(21)], 1)
    return v_out, j_out


# ===================================================================================================================== the gate
def floor_of(ref):
    """half an ulp of the fp32 output + 2^-140"""
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64) + TINY


def tolerance(ref, S, c):
    return c * U * np.asarray(S, np.float64) + floor_of(ref)


def ratio(got, ref, S):
    """max (|got - ref| - floor) / (2^-24 S) over the elements (0 where that is <= 0; inf for a non-finite got)"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float('inf')
    e = np.maximum(np.abs(got - ref) - floor_of(ref), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e > 0, e / (U * S), 0.0)
    return float(r.max())


def check(got, ref, S, c, what=''):
    """every element |got - ref| <= c 2^-24 S + floor; -> the largest ratio (in units of 2^-24 S)"""
    r = ratio(got, ref, S)
    if not r <= c:
        got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
        bad = ~(np.abs(got - ref) <= tolerance(ref, S, c))
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError('%s: %d of %d elements outside c 2^-24 S (c = %.3g, worst ratio %.4g); first at %s: got %.9g, ref %.9g, S %.4g'
                             % (what, int(bad.sum()), bad.size, c, r, i, got[i], ref[i], S[i]))
    return r


# ===================================================================================================================== case classes
JOINT_CLASSES = ('zero', 'eps', 'small', 'normal', 'pi', 'twopi', 'large', 'one_hot')
ROOT_CLASSES = ('normal', 'scaled', 'near_parallel', 'anti_parallel', 'sub_clamp', 'orthonormal', 'degenerate')
EXACT_JOINTS = ('zero', 'eps', 'pi', 'twopi', 'one_hot')          # need the 'ident' tables: the axis-angles themselves are the inputs
EPS_SET = (1e-10, 1e-9, 1e-8, 3e-8, 1e-7, 1e-6)
PAR_EPS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
# the loose tolerance exceeds 2^-8 max |verts| there (tests/test_mano_cases_ref.py re-checks the split)
PAR_EPS_DEGENERATE = {'near_parallel': (1e-4, 1e-5), 'anti_parallel': (1e-3, 1e-4, 1e-5)}


def _unit(r):
    v = r.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def joint_pose(cls, variant, r):
    """45 pose inputs (float32) of joint class `cls`; different joints / fingers of the hand get different members of the class"""
    f = np.float32
    if cls == 'zero':
        return np.zeros(45, f)
    if cls == 'eps':
        vals = np.array([s * e for e in EPS_SET for s in (1, -1)])
        aa = vals[(np.arange(45) * 5 + 7 * variant) % len(vals)].astype(f)
        aa[3 * (variant % 15)] = f(-1e-8)                     # aa + 1e-8 cancels to 0 in this component (fp32)
        return aa
    if cls == 'small':
        return (r.choice([-1, 1], 45) * 10.0 ** r.uniform(-4, -2, 45)).astype(f)
    if cls == 'normal':
        return r.normal(0, 0.7, 45).astype(f)
    if cls in ('pi', 'twopi'):
        base = np.pi if cls == 'pi' else 2 * np.pi
        rel = (0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -12, -2.0 ** -12)
        axes = [_unit(r) if j % 4 else np.eye(3)[j % 3] for j in range(15)]
        return np.concatenate([axes[j] * base * (1 + rel[(j + variant) % 5]) for j in range(15)]).astype(f)
    if cls == 'large':
        return np.concatenate([_unit(r) * r.uniform(10, 60) for _ in range(15)]).astype(f)
    if cls == 'one_hot':
        aa = np.zeros(45, f)
        j = (4 * variant + 2) % 15
        aa[3 * j:3 * j + 3] = (_unit(r) * (12.0 + 9 * variant)).astype(f)
        return aa
    raise KeyError(cls)


ROOT_VARIANTS = collections.OrderedDict([
    ('normal', ('a', 'b')), ('scaled', ('1e-5', '1e-7_30', '1e15')), ('near_parallel', PAR_EPS), ('anti_parallel', PAR_EPS),
    ('sub_clamp', ('x0.5', 'y0.5', 'x2', 'y2')), ('orthonormal', ('random', 'identity')), ('degenerate', ('parallel', 'zero_x', 'zero_y', 'both_zero'))])


def root_6d(cls, variant, r):
    """-> (six fp32 numbers, class after the 2^-8 condition)"""
    x, y = r.normal(0, 1, 3), r.normal(0, 1, 3)
    out = cls
    if cls == 'scaled':
        if variant == '1e-5':
            x, y = x * 1e-5, y * 1e-5
        elif variant == '1e-7_30':
            x, y = x * 1e-7, y / np.linalg.norm(y) * 30
        else:
            x, y = x * 1e15, y * 1e15
    elif cls in ('near_parallel', 'anti_parallel'):
        y = (1.5 if cls == 'near_parallel' else -1.5) * x + variant * y
        if variant in PAR_EPS_DEGENERATE[cls]:
            out = 'degenerate'
    elif cls == 'sub_clamp':
        ln = 0.5e-8 if variant.endswith('0.5') else 2e-8
        if variant[0] == 'x':
            x = x / np.linalg.norm(x) * ln
        else:
            y = y / np.linalg.norm(y) * ln
    elif cls == 'orthonormal':
        if variant == 'identity':
            x, y = np.array([1., 0, 0]), np.array([0., 1, 0])
        else:
            q, _ = np.linalg.qr(r.normal(0, 1, (3, 3)))
            x, y = q[:, 0], q[:, 1]
    elif cls == 'degenerate':
        if variant == 'parallel':
            x = np.array([0.5, -0.25, 1.0]); y = 2 * x
        elif variant == 'zero_x':
            x = np.zeros(3)
        elif variant == 'zero_y':
            y = np.zeros(3)
        else:
            x, y = np.zeros(3), np.zeros(3)
    return np.concatenate([x, y]).astype(np.float32), out


def _betas(i, r):
    if i % 3 == 0:
        return np.zeros(10, np.float32)
    if i % 3 == 1:
        return r.normal(0, 1, 10).astype(np.float32)
    b = np.zeros(10, np.float32)
    b[i % 10] = 3.0 if i % 2 else -3.0
    return b


CAM_S = (1.2, -0.7, 0.0, 1e3)
Case = collections.namedtuple('Case', 'name kind side center root_palm jc rc rvar para')


def _centre(i):
    return (-1, 0, 9, TIP_CENTRES[(i // 4) % 3])[i % 4]


def _make(prefix, i, side, jc, jvar, rc, rvar, root_palm=False, center=None):
    r = _rng('%s.%d.%s.%s.%s.%s' % (prefix, i, side, jc, rc, rvar))
    kind = 'ident' if jc in EXACT_JOINTS else 'pca'
    root, rc_out = root_6d(rc, rvar, r)
    cam = np.array([CAM_S[i % 4], r.normal(0, 0.3), r.normal(0, 0.3)], np.float32)
    para = np.concatenate([root, joint_pose(jc, jvar, r), _betas(i, r), cam]).astype(np.float32)
    c = _centre(i) if center is None else center
    return Case('%s%03d_%s_c%d%s_%s_%s_%s' % (prefix, i, side, c, 'p' if root_palm else '', jc, rc, rvar), kind, side, c, root_palm, jc, rc_out, str(rvar), para)


@functools.lru_cache(maxsize=None)
def forward_cases():
    """joint classes x 3 variants x 2 sides at a normal root, then every root variant x 2 sides at normal joints; centres -1, 0, 9 and a
    fingertip cycle, betas 0 / N(0,1) / +-3 one-hot cycle, cam scale 1.2 / -0.7 / 0 / 1e3 cycle; root_palm on every 5th case; a degenerate
    root on one side only (the 10 % cap)"""
    out, i = [], 0
    for jc in JOINT_CLASSES:
        for jvar in range(4):
            for side in ('left', 'right'):
                out.append(_make('f', i, side, jc, jvar, 'normal', 'a', root_palm=i % 5 == 4))
                i += 1
    for rc, variants in ROOT_VARIANTS.items():
        for rvar in variants:
            degenerate = rc == 'degenerate' or rvar in PAR_EPS_DEGENERATE.get(rc, ())
            for side in (('left', 'right')[i % 2],) if degenerate else ('left', 'right'):
                out.append(_make('f', i, side, 'normal', 0, rc, rvar, root_palm=i % 5 == 4))
                i += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def backward_cases():
    """the backward rejects root_palm; exactly-zero and exactly-parallel 6D columns are left out (the reference's autograd yields NaN
    there: sqrt at 0); of the degenerate eps only near_parallel 1e-4 stays (the 10 % cap)"""
    out, i = [], 0
    for jc in JOINT_CLASSES:
        for side in ('left', 'right'):
            out.append(_make('b', i, side, jc, i % 3, 'normal', 'a'))
            i += 1
    for rc, variants in ROOT_VARIANTS.items():
        for rvar in variants:
            if rvar in ('parallel', 'zero_x', 'zero_y', 'both_zero', 1e-5) or (rc, rvar) in (('normal', 'a'), ('anti_parallel', 1e-4)):
                continue
            out.append(_make('b', i, ('left', 'right')[i % 2], 'normal', 0, rc, rvar))
            i += 1
    return tuple(out)


def cotangents(case):
    """fp32 cotangents of the four outputs; the two candidate middle-finger tip vertices 444 / 445 get cotangents that tell them apart"""
    if case.name in _COT:
        return _COT[case.name]
    r = _rng('cot.' + case.name)
    cot = {'verts': r.normal(0, 1, (778, 3)), 'joints': r.normal(0, 1, (21, 3)), 'joint_uv': r.normal(0, 1, (21, 2)), 'mesh_uv': r.normal(0, 1, (778, 2))}
    cot['verts'][444] = (5.0, -4.0, 3.0)
    cot['verts'][445] = (-5.0, 4.0, -3.0)
    return {k: v.astype(np.float32) for k, v in cot.items()}


COT_SUBSETS = (KINDS, ('verts', 'joints'), ('joint_uv', 'mesh_uv'), ('verts',), ('joints',), ('joint_uv',), ('mesh_uv',))   # the engine's: all four, xyz only, uv only

GtCase = collections.namedtuple('GtCase', 'name kind side ncomps center new_skel jc root pose shape scale trans')


@functools.lru_cache(maxsize=None)
def gt_cases():
    """ncomps 1 / 7 / 12 / 45 / 0 (rotation matrices) x the centre classes, joint classes cycling (the exact ones at ncomps = 45 on the
    'ident' tables), scale / trans (0.7 m) on and off, new_skel on every third case, both sides"""
    out, i = [], 0
    for ncomps in (1, 7, 12, 45, 0):
        for ci in range(4):
            for side in ('left', 'right'):
                r = _rng('gt.%d' % i)
                jc = JOINT_CLASSES[i % 8] if ncomps in (45, 0) else ('small', 'normal', 'large')[i % 3]
                kind = 'ident' if (jc in EXACT_JOINTS and ncomps == 45) else 'pca'
                aa = joint_pose(jc, i % 3, r)
                if ncomps == 0:
                    with torch.no_grad():
                        pose = rodrigues_classic(torch.from_numpy(aa.astype(np.float64)).reshape(15, 3)).float().numpy().reshape(15, 3, 3)
                else:
                    pose = aa[:ncomps] * np.float32(3.0 if ncomps < 45 and jc == 'large' else 1.0)
                q, _ = np.linalg.qr(r.normal(0, 1, (3, 3)))
                root = (q * np.sign(np.linalg.det(q))).astype(np.float32)
                scale = np.float32((1.3, -0.6)[i % 2]) if i % 4 >= 2 else None
                trans = (_unit(r) * 0.7).astype(np.float32) if i % 3 != 1 else None
                c = _centre(ci + 4 * (i // 8))
                out.append(GtCase('g%03d_%s_n%d_c%d_%s' % (i, side, ncomps, c, jc), kind, side, ncomps, c, i % 3 == 0, jc, root, pose, _betas(i, r), scale, trans))
                i += 1
    return tuple(out)


# ===================================================================================================================== references
def _t(a, dt):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64)).to(dt)


_MEMO = {}


def _memo(f):
    """per case name: every reference is computed once and shared (the arrays are not to be written to)"""
    @functools.wraps(f)
    def g(case, *a, **kw):
        if kw.get('root_mat') is not None or any(isinstance(x, np.ndarray) for x in a):
            return f(case, *a, **kw)
        key = (f.__name__, case.name, a, tuple(sorted(kw.items())))
        if key not in _MEMO:
            _MEMO[key] = f(case, *a, **kw)
        return _MEMO[key]
    return g


@_memo
def forward_ref(case, dt=torch.float64, fold=False, mut=None, root_mat=None):
    """the four outputs of one case (numpy, sample dimension dropped)"""
    with torch.no_grad():
        out = mano_outputs(case.kind, case.side, case.center, _t(case.para[None], dt), case.root_palm, None if root_mat is None else _t(root_mat[None], dt), fold, mut)
    return {k: o[0].numpy() for k, o in zip(KINDS, out)}


@_memo
def forward_scale(case, root_mat=None):
    """S per element of the four outputs: the larger of the two orders' running bounds / u"""
    S = None
    with torch.no_grad():
        for fold in (False, True):
            out = mano_outputs(case.kind, case.side, case.center, V(_t(case.para[None], torch.float64)), case.root_palm,
                               None if root_mat is None else V(_t(root_mat[None], torch.float64)), fold)
            s = {k: o.e[0].numpy() / U for k, o in zip(KINDS, out)}
            S = s if S is None else {k: np.maximum(S[k], s[k]) for k in KINDS}
    return S


def root_f32(case):
    """the 3x3 root of the float32 numpy robust_rot6d: the op sequence the kernel promises"""
    return OM.robust_rot6d(case.para[None, :6].astype(np.float32))[0]


def flag_f32(case):
    """det < 0 of the float32 restatement's root (the reference asserts det >= 0, rot6d.py:50)"""
    R = root_f32(case).astype(np.float32)
    x, y, z = R[:, 0], R[:, 1], R[:, 2]
    f = np.float32
    det = f(f(x[0] * f(f(y[1] * z[2]) - f(z[1] * y[2]))) - f(y[0] * f(f(x[1] * z[2]) - f(z[1] * x[2])))) + f(z[0] * f(f(x[1] * y[2]) - f(y[1] * x[2])))
    return int(det < 0)


def oracle_f32(case):
    """(a): oracle/mano.py in float32 (no root_palm there: None for such cases)"""
    if case.root_palm:
        return None
    p = case.para[None].astype(np.float32)
    v, j = OM.mano_forward(tables(case.kind, case.side), p[:, :51], p[:, 51:61], case.side, None if case.center < 0 else case.center)
    return {'verts': v[0], 'joints': j[0], 'joint_uv': OM.projection_batch_xy(p[:, 61], p[:, 62:64], j)[0], 'mesh_uv': OM.projection_batch_xy(p[:, 61], p[:, 62:64], v)[0]}


def gt_args(case, dt, wrap=lambda x: x):
    w = lambda a: None if a is None else wrap(_t(np.asarray(a)[None], dt))  # noqa: E731
    return dict(root=w(case.root), pose=w(case.pose), shape=w(case.shape), ncomps=case.ncomps, center=case.center, scale=w(case.scale), trans=w(case.trans), new_skel=case.new_skel)


@_memo
def gt_ref(case, dt=torch.float64, fold=False, mut=None):
    with torch.no_grad():
        v, j = gt_outputs(case.kind, case.side, fold=fold, mut=mut, **gt_args(case, dt))
    return {'verts': v[0].numpy(), 'joints': j[0].numpy()}


@_memo
def gt_scale(case):
    S = None
    with torch.no_grad():
        for fold in (False, True):
            v, j = gt_outputs(case.kind, case.side, fold=fold, **gt_args(case, torch.float64, V))
            s = {'verts': v.e[0].numpy() / U, 'joints': j.e[0].numpy() / U}
            S = s if S is None else {k: np.maximum(S[k], s[k]) for k in s}
    return S


def gt_oracle_f32(case):
    from oracle import gt_mano as G
    b = tables(case.kind, case.side)
    T = {'hands_components': b['th_comps'], 'hands_mean': b['th_hands_mean'].reshape(45), 'J_regressor': b['th_J_regressor'], 'weights': b['th_weights'],
         'posedirs': b['th_posedirs'], 'v_template': b['th_v_template'].reshape(778, 3), 'shapedirs': b['th_shapedirs']}
    n = lambda a: None if a is None else np.asarray(a, np.float32)[None]  # noqa: E731
    v, j = G.gt_mano_forward(T, n(case.root), n(case.pose), n(case.shape), n(case.trans), None if case.scale is None else np.asarray([case.scale], np.float32),
                             None if case.center < 0 else case.center, case.ncomps > 0, case.new_skel)
    return {'verts': v[0], 'joints': j[0]}


_COT = {}             # cotangents given with a case (the G13 cases) instead of drawn by name
_BWD = {}


def backward_refs(case, dt=torch.float64, mut=None, fold=False):
    """{subset of KINDS: g para [64]}: the gradient of sum_k <cot_k, out_k> over each subset of COT_SUBSETS, by autograd through the restatement
    (one forward, one backward pass per subset)"""
    key = (case.name, dt, mut, fold)
    if key not in _BWD:
        cot = cotangents(case)
        p = _t(case.para[None], dt).requires_grad_(True)
        out = mano_outputs(case.kind, case.side, case.center, p, fold=fold, mut=mut)
        part = {k: (o[0] * _t(cot[k], dt)).sum() for k, o in zip(KINDS, out)}
        _BWD[key] = {kinds: torch.autograd.grad(sum(part[k] for k in kinds), p, retain_graph=True)[0][0].numpy() for kinds in COT_SUBSETS}
    return _BWD[key]


def backward_ref(case, kinds=KINDS, dt=torch.float64, mut=None, fold=False):
    return backward_refs(case, dt, mut, fold)[tuple(kinds)]


_ABS_JACOBIAN = {}


def backward_abs_jacobian(case):
    """A[kind][k] = sum_i |J_ik| |cot_i| per output kind (float64 forward-mode autograd, the 64 tangents as one batch): S of any subset of
    the cotangents is the sum of its kinds' A plus |g|"""
    import torch.autograd.forward_ad as fwAD
    if case.name not in _ABS_JACOBIAN:
        cot = cotangents(case)
        p = _t(case.para[None], torch.float64).repeat(64, 1)
        with fwAD.dual_level():
            out = mano_outputs(case.kind, case.side, case.center, fwAD.make_dual(p, torch.eye(64, dtype=torch.float64)))
            A = {}
            for kind, o in zip(KINDS, out):
                t = fwAD.unpack_dual(o).tangent
                A[kind] = (t.abs() * _t(cot[kind], torch.float64).abs()[None]).reshape(64, -1).sum(1).numpy()
        _ABS_JACOBIAN[case.name] = A
    return _ABS_JACOBIAN[case.name]


def backward_scale(case, kinds=KINDS):
    A = backward_abs_jacobian(case)
    return sum(A[k] for k in kinds) + np.abs(backward_ref(case, kinds))


G13_JOINT_CLASS = {'normal': 'normal', 'large': 'large', 'zero_pose': 'normal'}     # zero PCA coefficients: the axis-angles are hands_mean
G13_SEL = {'all': KINDS, 'verts': ('verts',), 'joints': ('joints',), 'joint_uv': ('joint_uv',), 'mesh_uv': ('mesh_uv',)}


def g13_cases():
    """the inputs of tests/golden/g13_mano_grad.npz (torch autograd through the reference's own modules) as cases: -> [(case, golden key prefix, sample)]"""
    from oracle.golden_inputs import MANO_GRAD_CASES, mano_grad_inputs
    out = []
    for side in ('left', 'right'):
        for name, center in MANO_GRAD_CASES:
            para, cot = mano_grad_inputs(name, side)
            for b in range(para.shape[0]):
                c = Case('g13_%s_%s_c%d_%d' % (side, name, center, b), 'pca', side, center, False, G13_JOINT_CLASS[name], 'normal', 'g13', para[b])
                _COT[c.name] = {k: v[b] for k, v in cot.items()}
                out.append((c, '%s_%s_c%d' % (side, name, center), b))
    return out


# ===================================================================================================================== measured constants
class one_thread(object):
    """the float32 references are measured on one thread: torch's float32 reductions change their order, and these ratios by a factor of
    up to 4, with the thread count, and RATIOS has to be reproducible"""
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


def nondegenerate(cases):
    return [c for c in cases if c.rc != 'degenerate']


def measure_forward():
    """-> (ratios per kind, ratios of the root-as-operand gate, the largest tolerance at c = 1 per kind in units of the sample's max |verts|
    -- of max(1, |s|) max |verts| for the two projections, whose unit is s times a length)"""
    R, Rt, tol = {k: 0.0 for k in KINDS}, {'verts': 0.0, 'joints': 0.0}, {k: 0.0 for k in KINDS}
    with one_thread():
        _measure_forward(R, Rt, tol)
    return R, Rt, tol


def _measure_forward(R, Rt, tol):
    for c in nondegenerate(forward_cases()):
        ref, S = forward_ref(c), forward_scale(c)
        refs32 = [r for r in (oracle_f32(c), forward_ref(c, torch.float32, fold=True)) if r is not None]
        vm = np.abs(ref['verts']).max()
        for k in KINDS:
            R[k] = max([R[k]] + [ratio(r[k], ref[k], S[k]) for r in refs32])
            tol[k] = max(tol[k], float(tolerance(ref[k], S[k], 1.0).max() / (vm * (max(1.0, abs(float(c.para[61]))) if k.endswith('uv') else 1.0))))
        Rm = root_f32(c)
        ref, S = forward_ref(c, root_mat=Rm), forward_scale(c, root_mat=Rm)
        refs32 = [r for r in (oracle_f32(c), forward_ref(c, torch.float32, fold=True, root_mat=Rm)) if r is not None]
        for k in Rt:
            Rt[k] = max([Rt[k]] + [ratio(r[k], ref[k], S[k]) for r in refs32])


def measure_gt():
    R = {'verts': 0.0, 'joints': 0.0}
    with one_thread():
        for c in gt_cases():
            ref, S = gt_ref(c), gt_scale(c)
            for r in (gt_oracle_f32(c), gt_ref(c, torch.float32, fold=True)):
                for k in R:
                    R[k] = max(R[k], ratio(r[k], ref[k], S[k]))
    return R


def measure_backward(g13=None):
    """-> {(column group, root class, joint class): ratio}; g13: the loaded tests/golden/g13_mano_grad.npz"""
    R = {}

    def acc(c, kinds, g32):
        g, S = backward_ref(c, kinds), backward_scale(c, kinds)
        for gr, sl in GROUPS.items():
            R[(gr, c.rc, c.jc)] = max(R.get((gr, c.rc, c.jc), 0.0), ratio(g32[sl], g[sl], S[sl]))
    with one_thread():
        for c in nondegenerate(backward_cases()):
            for kinds in COT_SUBSETS:
                for fold in (False, True):                      # float32 autograd through both orders of the restatement
                    acc(c, kinds, backward_ref(c, kinds, torch.float32, fold=fold))
        for c, pre, b in (g13_cases() if g13 is not None else ()):
            for sel, kinds in G13_SEL.items():
                acc(c, kinds, np.asarray(g13[pre + '.' + sel][b], np.float64))
                for fold in (False, True):
                    acc(c, kinds, backward_ref(c, kinds, torch.float32, fold=fold))
    return R


# the reference ratios (recorded 5 % above the measurement, three digits): forward / gt per output kind, backward per (column group, root
# class, joint class); c = MARGIN x ratio.  Re-measured by tests/test_mano_cases_ref.py.  The backward's S is a first-order scale, not a
# bound (it cannot see cancellation inside the chain rule), so its ratios exceed 1 where the function is stiff: (pca, twopi) is the tangential
# gradient at |aa| = 2 pi, where J itself vanishes with sin(half).
RATIOS = {
    'forward': {'verts': 0.0191, 'joints': 0.0482, 'joint_uv': 0.0477, 'mesh_uv': 0.0183},
    'forward_root_operand': {'verts': 0.0231, 'joints': 0.0238},
    'gt': {'verts': 0.0732, 'joints': 0.0554},
    'backward': {
        ('root', 'anti_parallel', 'normal'): 30.3, ('root', 'near_parallel', 'normal'): 641.0, ('root', 'normal', 'eps'): 2.02,
        ('root', 'normal', 'large'): 13.1, ('root', 'normal', 'normal'): 2.73, ('root', 'normal', 'one_hot'): 1.36,
        ('root', 'normal', 'pi'): 2.86, ('root', 'normal', 'small'): 9.05, ('root', 'normal', 'twopi'): 5.88,
        ('root', 'normal', 'zero'): 1.92, ('root', 'orthonormal', 'normal'): 0.825, ('root', 'scaled', 'normal'): 3.21,
        ('root', 'sub_clamp', 'normal'): 5.31,
        ('pca', 'anti_parallel', 'normal'): 30.7, ('pca', 'near_parallel', 'normal'): 823.0, ('pca', 'normal', 'eps'): 2.73,
        ('pca', 'normal', 'large'): 39.3, ('pca', 'normal', 'normal'): 4.57, ('pca', 'normal', 'one_hot'): 2.83,
        ('pca', 'normal', 'pi'): 10.4, ('pca', 'normal', 'small'): 3.28, ('pca', 'normal', 'twopi'): 230000.0,
        ('pca', 'normal', 'zero'): 1.9, ('pca', 'orthonormal', 'normal'): 3.31, ('pca', 'scaled', 'normal'): 4.25,
        ('pca', 'sub_clamp', 'normal'): 3.55,
        ('betas', 'anti_parallel', 'normal'): 27.2, ('betas', 'near_parallel', 'normal'): 505.0, ('betas', 'normal', 'eps'): 3.92,
        ('betas', 'normal', 'large'): 20.8, ('betas', 'normal', 'normal'): 6.35, ('betas', 'normal', 'one_hot'): 4.0,
        ('betas', 'normal', 'pi'): 6.81, ('betas', 'normal', 'small'): 3.73, ('betas', 'normal', 'twopi'): 3.51,
        ('betas', 'normal', 'zero'): 5.77, ('betas', 'orthonormal', 'normal'): 4.41, ('betas', 'scaled', 'normal'): 7.51,
        ('betas', 'sub_clamp', 'normal'): 5.73,
        ('cam_s', 'anti_parallel', 'normal'): 1.08, ('cam_s', 'near_parallel', 'normal'): 471.0, ('cam_s', 'normal', 'eps'): 0.411,
        ('cam_s', 'normal', 'large'): 11.1, ('cam_s', 'normal', 'normal'): 1.79, ('cam_s', 'normal', 'one_hot'): 0.372,
        ('cam_s', 'normal', 'pi'): 1.17, ('cam_s', 'normal', 'small'): 0.307, ('cam_s', 'normal', 'twopi'): 0.326,
        ('cam_s', 'normal', 'zero'): 1.13, ('cam_s', 'orthonormal', 'normal'): 1.51, ('cam_s', 'scaled', 'normal'): 0.688,
        ('cam_s', 'sub_clamp', 'normal'): 0.852,
        ('cam_t', 'anti_parallel', 'normal'): 0.316, ('cam_t', 'near_parallel', 'normal'): 0.547, ('cam_t', 'normal', 'eps'): 0.131,
        ('cam_t', 'normal', 'large'): 0.337, ('cam_t', 'normal', 'normal'): 0.3, ('cam_t', 'normal', 'one_hot'): 0.321,
        ('cam_t', 'normal', 'pi'): 0.382, ('cam_t', 'normal', 'small'): 0.426, ('cam_t', 'normal', 'twopi'): 0.318,
        ('cam_t', 'normal', 'zero'): 0.25, ('cam_t', 'orthonormal', 'normal'): 0.387, ('cam_t', 'scaled', 'normal'): 0.102,
        ('cam_t', 'sub_clamp', 'normal'): 0.184,
    },
}

MARGIN = 4.0      # the project's margin for another valid order: c = MARGIN x the recorded reference ratio


def c_of(table, key):
    return MARGIN * RATIOS[table][key]


# ===================================================================================================================== defects
Defect = collections.namedtuple('Defect', 'name family what')
DEFECTS = (
    Defect('left_tip_444', 'forward', 'left middle-finger tip taken from vertex 444 instead of 445'),
    Defect('angle_eps_outside', 'forward', '||aa|| + 1e-8 instead of ||aa + 1e-8||'),
    Defect('no_quat_renorm', 'forward', 'no quaternion re-normalisation'),
    Defect('pose_map_is_R', 'forward', 'pose map R instead of R - I'),
    Defect('level2_parent_of_neighbour', 'forward', "level-2 parent taken from the neighbouring finger"),
    Defect('centre_on_next_joint', 'forward', 'centring on joint c + 1'),
    Defect('vertex_196_unskinned', 'forward', 'vertex 196 (the first vertex of part 1) left at its unskinned value'),
    Defect('ty_used_for_u', 'forward', 'ty used for u'),
    Defect('root_palm_vertex_21', 'forward', 'root_palm with vertex 21 instead of 22'),
    Defect('gt_left_tip_445', 'gt', 'ground truth: tip 445 on the left hand'),
    Defect('gt_scale_before_centre', 'gt', 'ground truth: (v - c) s + t applied as (v s - c) + t'),
    Defect('gt_new_skel_wrong_pair', 'gt', 'ground truth: new_skel joint 9 from the vertex pair (271, 221)'),
    Defect('bwd_no_chain_carry', 'backward', 'no carry from grandchild to parent in the chain'),
    Defect('bwd_centre_sum_dropped', 'backward', "the centre joint's - sum g dropped"),
    Defect('bwd_tip_cotangent_dropped', 'backward', 'tip cotangent not added to its vertex'),
    Defect('bwd_cam_s_without_joint_uv', 'backward', 'g cam s without the joint_uv term'),
    Defect('bwd_angle_without_eps', 'backward', 'vx instead of vx + 1e-8 in g angle'),
    Defect('bwd_no_pose_blend', 'backward', 'pose-blend term not added to g R'),
    Defect('bwd_betas_without_joints', 'backward', 'g betas without the j_shapedirs term'),
    Defect('bwd_clamp_projects', 'backward', 'the clamped branch of the normalisation projects (mano_bwd.hip before this gate)'),
)


# Defects no fp32 gate can reject, with the reason; defect_report() measures them at <= 1 (in units of the tolerance) and the CPU test pins that.
EQUIVALENT = {
    'angle_eps_outside': 'q = (cos(a/2), sin(a/2) aa / a): sin(a/2) / a -> 1/2 for small a whatever a is, and for a >> 1e-8 the two angles differ by '
                         '1e-8 rad, a sixth of 2^-24 relative; measured 0.005 of the tolerance',
    'no_quat_renorm': '|q|^2 - 1 = sin^2(a/2) (|aa|^2 / |aa + 1e-8|^2 - 1) <= 1e-8 for a >> 1e-8 and <= a^2 / 4 below; measured 0.0014 of the tolerance',
    'bwd_angle_without_eps': 'changes g aa by g_angle 1e-8 / a, and g_angle = O(a) where a ~ 1e-8 (the rotation does not depend on the angle there), so the '
                             'change is <= 1e-8 relative; measured 0.92 of the (pca, normal, eps) tolerance, whose c = 4 x 2.73',
}
# root_palm_vertex_21: the old suite checked root_palm only through joint 0 == 0 after centring on it, which any vertex pair satisfies.
OLD_SUITE_BLIND = ('root_palm_vertex_21',)
# the defects the old gates' formulas accept on the benign cases of this list (normal root, normal joints): the three above and the clamp branch
OLD_GATES_ACCEPT = ('angle_eps_outside', 'no_quat_renorm', 'bwd_angle_without_eps', 'bwd_clamp_projects')


def defects():
    return DEFECTS


def _benign(c):
    return c.jc == 'normal' and c.rc == 'normal'


def defect_report(d):
    """-> (worst ratio of the defect over the list in units of c 2^-24 S, i.e. rejected iff > 1; whether the old max-norm gates accept it on
    the benign cases of the list)"""
    worst, old_ok = 0.0, True
    if d.family == 'forward':
        for c in nondegenerate(forward_cases()):
            ref, S, got = forward_ref(c), forward_scale(c), forward_ref(c, mut=d.name)
            for k in KINDS:
                worst = max(worst, ratio(got[k], ref[k], S[k]) / c_of('forward', k))
                if _benign(c) and np.abs(got[k] - ref[k]).max() >= (2e-6 if k.endswith('uv') else 1e-7):
                    old_ok = False
    elif d.family == 'gt':
        for c in gt_cases():
            ref, S, got = gt_ref(c), gt_scale(c), gt_ref(c, mut=d.name)
            for k in ('verts', 'joints'):
                worst = max(worst, ratio(got[k], ref[k], S[k]) / c_of('gt', k))
                if c.jc == 'normal' and np.abs(got[k] - ref[k]).max() >= 1.2e-7:
                    old_ok = False
    else:
        for c in nondegenerate(backward_cases()):
            for kinds in COT_SUBSETS:
                g, S, got = backward_ref(c, kinds), backward_scale(c, kinds), backward_ref(c, kinds, mut=d.name)
                for gr, sl in GROUPS.items():
                    worst = max(worst, ratio(got[sl], g[sl], S[sl]) / c_of('backward', (gr, c.rc, c.jc)))
                if _benign(c) and np.abs(got - g).max() / np.abs(g).max() >= 1e-5:
                    old_ok = False
    return worst, old_ok
