"""GPU: the MANO forward (dir_mano_forward, dir_mano_forward_pair), ground-truth (dir_gt_mano_forward) and backward
(dir_mano_backward_pair) kernels per element, at the case classes of tests/helpers/mano_cases.py (float64 references, error scales S and
constants c measured on float32 references -- never on the kernels -- are described and pinned there and in tests/test_mano_cases_ref.py).

Every launch shape of the forward is met: 1 and 4 vertex parts, 1 and 2 hands, rep = 8 / (hands * parts) in {8, 4, 2, 1} at batch sizes whose
group counts are no multiples of it, 2 and 4 samples per workgroup (DIR_MANO_SPW, child processes) -- and the kernel's promise of bit-identical
results across them is checked bit for bit.

Measured on the MI355X (information, not a bound; in units of 2^-24 S, c in brackets): forward verts 0.0181 (0.0764), joints 0.0458 (0.193),
joint_uv 0.0454 (0.191), mesh_uv 0.0174 (0.0732); root as operand verts 0.022 (0.0924), joints 0.0173 (0.0952) -- the promise of the reference's
op sequence held on every near-parallel, anti-parallel and sub-clamp root; ground truth verts 0.0642 (0.293), joints 0.0527 (0.222); backward at
most 0.63 c over every (column group, root class, joint class).  Every bit-equality held.  One defect was found: the backward's normalisation
projected in the clamped branch (6D root gradient of a column of length 0.5e-8: 3.4e4 c before the fix, 0.21 c after)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dir_amd import _capi
from dir_amd import functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import mano_cases as M  # noqa: E402
import mano_gpu_run as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = M.KINDS + ('flags',)


@pytest.fixture(scope='module')
def canonical():
    """every forward case run ALONE (B = 1, one hand): the bits every other launch shape must reproduce"""
    return {c.name: {k: a[0] for k, a in R.forward_single([c]).items()} for c in M.forward_cases()}


def _shaped(k, a):
    return a.reshape({'verts': (778, 3), 'joints': (21, 3), 'joint_uv': (21, 2), 'mesh_uv': (778, 2)}[k])


def test_forward_per_element(canonical):
    """loose gate (6D root as the operand), tight gate (root as operand: the float32 numpy robust_rot6d), flags; degenerate roots: finite + flag"""
    worst, worst_tight = {k: 0.0 for k in M.KINDS}, {'verts': 0.0, 'joints': 0.0}
    for c in M.forward_cases():
        got = canonical[c.name]
        assert int(got['flags']) == M.flag_f32(c), c.name
        if c.rc == 'degenerate':
            assert all(np.isfinite(got[k]).all() for k in M.KINDS), c.name
            continue
        ref, S = M.forward_ref(c), M.forward_scale(c)
        for k in M.KINDS:
            worst[k] = max(worst[k], M.check(_shaped(k, got[k]), ref[k], S[k], M.c_of('forward', k), '%s %s' % (c.name, k)))
        Rm = M.root_f32(c)
        ref, S = M.forward_ref(c, root_mat=Rm), M.forward_scale(c, root_mat=Rm)
        for k in worst_tight:
            worst_tight[k] = max(worst_tight[k], M.check(_shaped(k, got[k]), ref[k], S[k], M.c_of('forward_root_operand', k), '%s %s root as operand' % (c.name, k)))
    print('forward worst ratios (units of 2^-24 S):', {k: '%.3g (c %.3g)' % (worst[k], M.c_of('forward', k)) for k in worst},
          '; root as operand:', {k: '%.3g (c %.3g)' % (worst_tight[k], M.c_of('forward_root_operand', k)) for k in worst_tight})


def test_forward_bits_across_batches_strides_and_repeats(canonical):
    """the same sample gives the same bits alone, in a second run, and at every position of every batch size (parameters at strides 64 and 70)"""
    for i, (key, cs) in enumerate(R.by_config(M.forward_cases()).items()):
        again = R.forward_single([cs[0]], 70)
        assert all(R.same_bits(again[k][0], canonical[cs[0].name][k]) for k in KINDS), cs[0].name
        for B in R.BATCHES[1:]:
            for batch in R.batches(cs, B):
                r = R.forward_single(batch, 64 if (i + B) % 2 else 70)
                for n, c in enumerate(batch):
                    for k in KINDS:
                        assert R.same_bits(r[k][n], canonical[c.name][k]), (c.name, B, n, k)


def test_forward_pair_bits(canonical):
    """dir_mano_forward_pair, different cases (and configurations) per hand: every case as hand 0 and as hand 1, with the projections and with
    cam_lr / joint_uv_lr / mesh_uv_lr / flags_lr all NULL; one mano_forward_kernel launch per call (asserted by the runner)"""
    cfgs = list(R.by_config(M.forward_cases()).values())
    for i, a in enumerate(cfgs):
        b = cfgs[(i + 1) % len(cfgs)]
        B = R.BATCHES[i % len(R.BATCHES)]
        n = max(len(R.batches(a, B)), len(R.batches(b, B)))
        for projections in (True, False):
            for s in range(n):
                pair = [R.batches(a, B)[s % len(R.batches(a, B))], R.batches(b, B)[s % len(R.batches(b, B))]]
                r = R.forward_pair(pair, 70 if i % 2 else 64, projections)
                for h in (0, 1):
                    for m, c in enumerate(pair[h]):
                        for k in r[h]:
                            assert R.same_bits(r[h][k][m], canonical[c.name][k]), (c.name, 'hand %d' % h, B, m, k, projections)


def test_forward_one_part_large_batches_equal_the_four_part_bits(canonical):
    """B * hands >= 1024 runs one vertex part (640 threads): B = 1024 single hand and B = 512 pair, centre 0, against the 4-part bits"""
    cfgs = [cs for key, cs in R.by_config(M.forward_cases()).items() if key[2] == 0 and not key[3]]
    assert len(cfgs) >= 2
    for cs in cfgs[:2]:
        r = R.forward_single(R.batches(cs, 1024)[0])
        for n, c in enumerate(cs):
            assert all(R.same_bits(r[k][n], canonical[c.name][k]) for k in KINDS), (c.name, 1024)
            assert all(R.same_bits(r[k][1024 - len(cs) + n], r[k][(1024 - len(cs) + n) % len(cs)]) for k in KINDS)      # ... and the last cycle
    r = R.forward_pair([R.batches(cfgs[0], 512)[0], R.batches(cfgs[1], 512)[0]])
    for h in (0, 1):
        for n, c in enumerate(cfgs[h]):
            assert all(R.same_bits(r[h][k][n], canonical[c.name][k]) for k in KINDS), (c.name, 512, h)


def test_forward_samples_per_workgroup(tmp_path):
    """DIR_MANO_SPW is read once per process: one child per value (2, 4), one at a time, each under its own time limit, runs the sweep of
    R.spw_sweep (B = 5 and 9: a group's tail recomputes sample B - 1 and must write nothing -- the guard rows) and the parent compares bit for bit"""
    mine = R.spw_sweep()
    for spw in ('2', '4'):
        out = str(tmp_path / ('spw%s.npz' % spw))
        env = dict(os.environ, DIR_MANO_SPW=spw)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'mano_gpu_run.py'), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and 'OK' in r.stdout, 'DIR_MANO_SPW=%s child: exit %s\n%s%s' % (spw, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        theirs = np.load(out)
        assert set(theirs.files) == set(mine)
        for k, a in mine.items():
            assert R.same_bits(a, theirs[k]), (spw, k)


# ===================================================================================================================== ground truth
def _gt_run(cases):
    """cases of one (kind, side, ncomps, center, new_skel, scale?, trans?) configuration through dir_gt_mano_forward, with guard rows"""
    c0, B = cases[0], len(cases)
    T = R.packed(c0.kind, c0.side, -1)
    dev = lambda xs, shape: None if xs[0] is None else torch.from_numpy(np.stack([np.asarray(x, np.float32) for x in xs]).reshape(shape)).cuda()  # noqa: E731
    root, shape = dev([c.root for c in cases], (B, 9)), dev([c.shape for c in cases], (B, 10))
    pose = dev([c.pose for c in cases], (B, c0.ncomps if c0.ncomps else 135))
    scale, trans = dev([c.scale for c in cases], (B,)), dev([c.trans for c in cases], (B, 3))
    ins = [t for t in (root, shape, pose, scale, trans) if t is not None]
    befores = [t.clone() for t in ins]
    verts, joints = torch.full((B + 1, 2334), R.FILL, device='cuda'), torch.full((B + 1, 63), R.FILL, device='cuda')
    _capi.lib().dir_launch_log_reset()
    _capi.check(_capi.lib().dir_gt_mano_forward(T, _capi.ptr(root), _capi.ptr(pose), c0.ncomps, _capi.ptr(shape), _capi.ptr(trans), _capi.ptr(scale), c0.center,
                                                1 if c0.new_skel else 0, _capi.ptr(verts), _capi.ptr(joints), B, _capi.stream_ptr()), 'dir_gt_mano_forward')
    assert R.launched() == ['gt_mano_kernel']
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, befores)) and bool((verts[B:] == R.FILL).all()) and bool((joints[B:] == R.FILL).all())
    return {'verts': verts[:B].cpu().numpy(), 'joints': joints[:B].cpu().numpy()}


def test_ground_truth_per_element_and_bits():
    groups = {}
    for c in M.gt_cases():
        groups.setdefault((c.kind, c.side, c.ncomps, c.center, c.new_skel, c.scale is None, c.trans is None), []).append(c)
    worst = {'verts': 0.0, 'joints': 0.0}
    for cs in groups.values():
        alone = {c.name: _gt_run([c]) for c in cs}
        for c in cs:
            ref, S = M.gt_ref(c), M.gt_scale(c)
            for k in worst:
                worst[k] = max(worst[k], M.check(_shaped(k, alone[c.name][k][0]), ref[k], S[k], M.c_of('gt', k), '%s %s' % (c.name, k)))
            again = _gt_run([c])
            assert all(R.same_bits(again[k], alone[c.name][k]) for k in worst), c.name
        for B in (3, 17):
            for batch in R.batches(cs, B):
                r = _gt_run(batch)
                for n, c in enumerate(batch):
                    assert all(R.same_bits(r[k][n], alone[c.name][k][0]) for k in worst), (c.name, B, n)
    print('ground truth worst ratios (units of 2^-24 S):', {k: '%.3g (c %.3g)' % (worst[k], M.c_of('gt', k)) for k in worst})


# ===================================================================================================================== backward
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cots(cases, kinds):
    return {'g_' + k: _dev(np.stack([M.cotangents(c)[k] for c in cases])) for k in kinds}


def _backward_abi(cases_lr, kinds, stride, cam=True, g_cam=True):
    """dir_mano_backward_pair through the C ABI: 1 or 2 hands (one config each), gradients written at `stride` into a buffer of FILL with a guard row"""
    hands, B = len(cases_lr), len(cases_lr[0])
    P = C.c_void_p * hands
    Ts = (_capi.ManoTables * hands)(*[R.packed(*R.config(cs[0])) for cs in cases_lr])
    ps = [_dev(np.stack([c.para for c in cs])) for cs in cases_lr]
    befores = [p.clone() for p in ps]
    cots = [_cots(cs, kinds) for cs in cases_lr]
    outs = [torch.full((B + 1, stride), R.FILL, device='cuda') for _ in range(hands)]
    off = lambda ts, o: P(*[t.data_ptr() + 4 * o for t in ts])  # noqa: E731
    g = lambda k: P(*[ct['g_' + k].data_ptr() for ct in cots]) if k in kinds else None  # noqa: E731
    _capi.lib().dir_launch_log_reset()
    _capi.check(_capi.lib().dir_mano_backward_pair(Ts, off(ps, 0), 64, off(ps, 51), 64, off(ps, 61) if cam else None, 64, g('verts'), g('joints'), g('joint_uv'),
                                                   g('mesh_uv'), off(outs, 0), stride, off(outs, 51), stride, off(outs, 61) if g_cam else None, stride,
                                                   hands, B, _capi.stream_ptr()), 'dir_mano_backward_pair')
    assert R.launched() == ['mano_backward_kernel']
    torch.cuda.synchronize()
    res = []
    for o, p, b0 in zip(outs, ps, befores):
        assert torch.equal(p, b0) and bool((o[B:] == R.FILL).all()) and bool((o[:B, 64:] == R.FILL).all()), 'guard / parameter buffer written'
        if not g_cam:
            assert bool((o[:B, 61:64] == R.FILL).all()), 'cam gradient written though g_cam was NULL'
        res.append(o[:B, :64].cpu().numpy())
    return res


@pytest.fixture(scope='module')
def backward_alone():
    """every backward case alone through F.mano_backward (one hand, stride 64), every cotangent subset"""
    out = {}
    for c in M.backward_cases():
        T, p = R.packed(*R.config(c)), _dev(c.para[None])
        for kinds in M.COT_SUBSETS:
            out[c.name, kinds] = F.mano_backward([T], [p], **{k: [v] for k, v in _cots([c], kinds).items()})[0].cpu().numpy()[0]
    return out


def test_backward_per_element(backward_alone):
    """per column group (6D root, PCA, betas, cam scale, cam translation), every subset of cotangents the engine uses and each one alone"""
    worst, failures = {}, []
    for c in M.backward_cases():
        for kinds in M.COT_SUBSETS:
            got = backward_alone[c.name, kinds]
            if c.rc == 'degenerate':
                assert np.isfinite(got).all(), c.name
                continue
            g, S = M.backward_ref(c, kinds), M.backward_scale(c, kinds)
            for gr, sl in M.GROUPS.items():
                key = (gr, c.rc, c.jc)
                r = M.ratio(got[sl], g[sl], S[sl])
                worst[key] = max(worst.get(key, 0.0), r / M.c_of('backward', key))
                if not r <= M.c_of('backward', key):
                    failures.append('%s %s %s: ratio %.4g > c %.4g' % (c.name, '+'.join(kinds), gr, r, M.c_of('backward', key)))
    print('backward worst ratio / c per (column group, root class, joint class):', {k: '%.3g' % v for k, v in sorted(worst.items())})
    assert not failures, '\n'.join(failures[:40])


def test_backward_bits_across_batches_hands_strides_and_nulls(backward_alone):
    cfgs = list(R.by_config(M.backward_cases()).values())
    for i, cs in enumerate(cfgs):
        kinds = M.COT_SUBSETS[i % len(M.COT_SUBSETS)]
        for B in (1, 3, 17):
            for batch in R.batches(cs, B):
                r = _backward_abi([batch], kinds, 70 if B != 3 else 64)[0]                       # second run (B = 1) and batch independence
                for n, c in enumerate(batch):
                    assert R.same_bits(r[n], backward_alone[c.name, kinds]), (c.name, kinds, B, n)
        other = cfgs[(i + 1) % len(cfgs)]
        B = (1, 3, 17)[i % 3]
        pair = [R.batches(cs, B)[0], R.batches(other, B)[0]]
        r = _backward_abi(pair, M.KINDS, 64 if i % 2 else 70)                                    # two hands, different configurations
        rf = F.mano_backward([R.packed(*R.config(cs[0])) for cs in pair], [_dev(np.stack([c.para for c in cs])) for cs in pair],
                             **{k: [_cots(cs, M.KINDS)[k] for cs in pair] for k in ('g_verts', 'g_joints', 'g_joint_uv', 'g_mesh_uv')})     # ... through F, hands = 2
        for h in (0, 1):
            assert R.same_bits(rf[h].cpu().numpy(), r[h])
            for n, c in enumerate(pair[h]):
                assert R.same_bits(r[h][n], backward_alone[c.name, M.KINDS]), (c.name, 'hand %d' % h, B, n)
        xyz = ('verts', 'joints')
        batch = R.batches(cs, 3)[0]
        r = _backward_abi([batch], xyz, 70, cam=False)[0]                                        # cam NULL: the cam slot stays zero
        q = _backward_abi([batch], M.KINDS, 70, g_cam=False)[0]                                  # g_cam NULL: nothing written there (asserted inside)
        for n, c in enumerate(batch):
            assert R.same_bits(r[n][:61], backward_alone[c.name, xyz][:61]) and not r[n][61:].any(), (c.name, 'cam NULL')
            assert R.same_bits(q[n][:61], backward_alone[c.name, M.KINDS][:61]), (c.name, 'g_cam NULL')
