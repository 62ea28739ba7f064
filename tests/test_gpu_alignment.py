"""GPU: dir_procrustes_align / dir_point_set_nn / dir_threshold_counts (csrc/alignmetric.hip) and utils.alignment.AlignedMetrics held to the
float64 numpy restatement tests/helpers/alignment_ref.py, which tests/test_alignment_ref.py checks against closed forms; then the wiring
into apps.eval and apps.train.validate.

Inputs: 64 seeded pairs (alignment_ref.pairs: gt = the synthetic right template + 3 mm noise, pd = s Q (gt + 8 mm noise) + t, every eighth
pair mirrored in x), each at N = 778 and at a 21-point subset, alone (B = 1) and as a row of a B = 64 batch; every pair's problem is well
posed (the singular-value gap of its covariance, relative to sigma_1, is at least 1e-2: the smallest is 0.187).

Measured on the MI355X, largest absolute difference from the restatement:
    aligned positions and errors   9.69e-8 m over the 64 pairs (N = 778 and 21, alone and as rows of 64), 6.03e-8 m over the closed-form
                                   cases, 9.75e-8 m over the accumulator test's 48 pairs per hand (8.09e-8 m for the aligned joints)
    nearest-neighbour distances    5.63e-9 m
    transform (not gated itself)   s 5.8e-7, R 5.9e-7, t 7.8e-8 m
The gates are 4 x the largest measured values, for float32 sums taken in another order: 3.9e-7 m for positions and 2.25e-8 m for the
neighbour distances, both under the cap of 1e-6 m.
Counts must equal the restatement's except for values whose float64 error lies within the position gate of a threshold; at most 1 % of a
test's values may be left out that way."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import alignment_ref as R  # noqa: E402
from fake_split import write_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.utils import alignment as AL  # noqa: E402

pytestmark = pytest.mark.gpu

POS_MEASURED, NN_MEASURED = 9.752e-8, 5.633e-9
CAP = 1e-6
POS_GATE, NN_GATE = min(4 * POS_MEASURED, CAP), min(4 * NN_MEASURED, CAP)
BAND = POS_GATE
ROT_TOL = 1e-5
SUB = list(R.SUBSET21)


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def run_align(pd, gt, scale=True):
    out = AL.procrustes_align(dev(pd), dev(gt), scale=scale, want_aligned=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_nn(a, b):
    d_ab, d_ba = AL.nn_distances(dev(a), dev(b))
    torch.cuda.synchronize()
    return d_ab.cpu().numpy(), d_ba.cpu().numpy()


def check_rotation(tr, what):
    Rm = tr[1:10].astype(np.float64).reshape(3, 3)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < ROT_TOL and abs(np.linalg.det(Rm) - 1) < ROT_TOL, what


def check_fit(ref, got, row, what):
    """one sample against the restatement -> (position error, err error, transform differences (s, R, t))"""
    al, e, tr = got['aligned'][row].astype(np.float64), got['err'][row].astype(np.float64), got['transform'][row].astype(np.float64)
    ep, ee = np.abs(al - ref['aligned']).max(), np.abs(e - ref['err']).max()
    dt = (abs(tr[0] - ref['s']), np.abs(tr[1:10].reshape(3, 3) - ref['R']).max(), np.abs(tr[10:] - ref['t']).max())
    print('%s: max |aligned - ref| = %.3e m, max |err - ref| = %.3e m, transform: s %.2e, R %.2e, t %.2e m' % ((what, ep, ee) + dt))
    check_rotation(got['transform'][row], what)
    return ep, ee, dt


@pytest.fixture(scope='module')
def pairs():
    return R.pairs(64)


@pytest.fixture(scope='module')
def refs(pairs):
    pd, gt = pairs
    out = {}
    for name, idx in (('778', slice(None)), ('21', SUB)):
        out[name] = [R.procrustes(pd[i][idx], gt[i][idx]) for i in range(len(pd))]
        for i, r in enumerate(out[name]):
            assert r['det_fix'] == (i % 8 == 7)
        gap = min(R.well_posed(r) for r in out[name])
        print('N = %s: smallest singular-value gap %.3f' % (name, gap))
        assert gap >= 1e-2
    return out


def test_alignment_matches_the_restatement(pairs, refs):
    pd, gt = pairs
    worst, worst_t = [], []
    for name, idx in (('778', slice(None)), ('21', SUB)):
        p, g = pd[:, idx], gt[:, idx]
        got64 = run_align(p, g)
        for i in range(len(p)):
            alone = run_align(p[i:i + 1], g[i:i + 1])
            ep, ee, dt = check_fit(refs[name][i], alone, 0, 'N = %s pair %d alone' % (name, i))
            worst.append(max(ep, ee))
            worst_t.append(dt)
            for k in alone:
                assert np.array_equal(alone[k][0], got64[k][i]), (name, k, i)          # the same bits as a row of the batch
        ep, ee, _ = max(check_fit(refs[name][i], got64, i, 'N = %s pair %d as row of 64' % (name, i)) for i in (0, 7, 63))
        worst.append(max(ep, ee))
    wt = np.array(worst_t).max(0)
    print('MEASURED: positions %.3e m (gate %.3e m); transform: s %.3e, R %.3e, t %.3e m' % (max(worst), POS_GATE, wt[0], wt[1], wt[2]))
    assert max(worst) < POS_GATE


def closed_cases():
    """name -> (pd, gt, scale, check(ref)) in float64; the device sees the float32 roundings, which the restatement is given too"""
    g = np.random.default_rng(11)
    cloud = g.normal(0, 0.05, (50, 3)) * [1.0, 0.6, 0.3]
    Q = R.random_rotation(g)
    pm_pd, pm_gt, _ = R.planar_mirror()
    return {'exact': (cloud, 1.3 * cloud @ Q.T + [0.1, -0.05, 0.4], True),
            'mirrored': (cloud, cloud * [-1.0, 1.0, 1.0] + [0.1, 0, 0], True),
            'planar_mirror': (pm_pd, pm_gt, True),
            'scale_off': (cloud, 1.7 * cloud @ Q.T + [0.3, 0.1, -0.2], False)}


def test_closed_form_cases_on_the_device():
    worst = 0.0
    for name, (pd, gt, scale) in closed_cases().items():
        pd, gt = pd.astype(np.float32), gt.astype(np.float32)
        ref = R.procrustes(pd, gt, scale=scale)
        got = run_align(pd[None], gt[None], scale=scale)
        ep, ee, _ = check_fit(ref, got, 0, name)
        worst = max(worst, ep, ee)
        assert ep < POS_GATE and ee < POS_GATE, name
        if name in ('exact', 'planar_mirror'):
            assert got['err'].max() < POS_GATE, name                                   # the zero error of the closed form
        if name == 'mirrored':
            assert got['err'].mean() > 0.005 and ref['det_fix']
        if name == 'planar_mirror':
            assert abs(np.trace(got['transform'][0, 1:10].reshape(3, 3)) + 1) < ROT_TOL     # a flip: a rotation by pi
        if name == 'scale_off':
            assert got['transform'][0, 0] == 1.0 and got['err'].max() > 0.01
    print('MEASURED: closed-form cases %.3e m' % worst)


def test_two_runs_and_any_batch_give_identical_bits(pairs):
    pd, gt = pairs
    for idx in (slice(None), SUB):
        p, g = pd[:, idx], gt[:, idx]
        a, b = run_align(p, g), run_align(p, g)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        rows = [3, 15, 40, 62, 9]
        c = run_align(p[rows], g[rows])
        for j, r in enumerate(rows):
            assert all(np.array_equal(c[k][j], a[k][r]) for k in a), r
        lean = AL.procrustes_align(dev(p), dev(g))
        assert sorted(lean) == ['err', 'transform'] and np.array_equal(lean['err'].cpu().numpy(), a['err'])
        n1, n2 = run_nn(a['aligned'], g), run_nn(a['aligned'], g)
        assert np.array_equal(n1[0], n2[0]) and np.array_equal(n1[1], n2[1])
        n3 = run_nn(a['aligned'][rows], g[rows])
        assert np.array_equal(n3[0], n1[0][rows]) and np.array_equal(n3[1], n1[1][rows])


def test_degenerate_samples_are_nan_and_leave_their_neighbours_alone(pairs):
    pd, gt = pairs
    for idx in (slice(None), SUB):
        p, g = pd[:8, idx].copy(), gt[:8, idx].copy()
        clean = run_align(p, g)
        p[2, 5, 1] = np.nan                        # a NaN in the prediction
        g[4, 0, 2] = np.inf                        # a non-finite ground truth
        p[6] = p[6, 3]                             # all points equal
        got = run_align(p, g)
        for r in (2, 4, 6):
            assert all(np.isnan(got[k][r]).all() for k in got), r
        for r in (0, 1, 3, 5, 7):
            assert all(np.array_equal(got[k][r], clean[k][r]) for k in got), r
        # collinear points: some maximiser, finite and a proper rotation
        line = (np.linspace(0, 1, p.shape[1])[:, None] * [[0.1, 0.2, -0.1]]).astype(np.float32)
        col = run_align(line[None], g[:1])
        assert np.isfinite(col['aligned']).all() and np.isfinite(col['err']).all()
        check_rotation(col['transform'][0], 'collinear')


def test_nearest_neighbour_distances(pairs):
    pd, gt = pairs
    al = run_align(pd, gt)['aligned']
    worst = 0.0
    d_ab, d_ba = run_nn(al, gt)
    for i in range(0, 64, 7):
        ra, rb = R.nn(al[i], gt[i])
        worst = max(worst, np.abs(d_ab[i] - ra).max(), np.abs(d_ba[i] - rb).max())
    same = run_nn(gt, gt)
    assert (same[0] == 0).all() and (same[1] == 0).all()                    # identical sets: exactly 0
    # Na != Nb
    a, b = al[:4, :300], gt[:4, 100:]
    x, y = run_nn(a, b)
    assert x.shape == (4, 300) and y.shape == (4, 678)
    for i in range(4):
        ra, rb = R.nn(a[i], b[i])
        worst = max(worst, np.abs(x[i] - ra).max(), np.abs(y[i] - rb).max())
    # N = 4096 against 3000: two LDS chunks of targets, four query points per thread
    g = np.random.default_rng(5)
    big_a, big_b = g.normal(0, 0.05, (2, 4096, 3)).astype(np.float32), g.normal(0, 0.05, (2, 3000, 3)).astype(np.float32)
    big_b[1, 2999] = big_a[1, 4095]                                          # the last of each set meet
    x, y = run_nn(big_a, big_b)
    assert x[1, 4095] == 0 and y[1, 2999] == 0
    for i in range(2):
        ra, rb = R.nn(big_a[i], big_b[i])
        worst = max(worst, np.abs(x[i] - ra).max(), np.abs(y[i] - rb).max())
    x, y = run_nn(big_a, big_a[:, ::-1].copy())
    assert (x == 0).all() and (y == 0).all()
    # non-finite points: a query point gives NaN, a target point is passed over
    bad = gt[:2].copy()
    bad[0, 10] = np.nan
    x, y = run_nn(bad, gt[:2])
    assert np.isnan(x[0, 10]) and np.isfinite(np.delete(x[0], 10)).all() and np.isfinite(y).all() and (x[1] == 0).all()
    assert y[0, 10] > 0 and (np.delete(y[0], 10) == 0).all()
    print('MEASURED: nearest-neighbour distances %.3e m (gate %.3e m)' % (worst, NN_GATE))
    assert worst < NN_GATE


def bracket(e64, t, band=BAND):
    """-> (lowest, highest) counts the device may give for the float64 errors e64, and the share of values within the band of a threshold"""
    e = np.asarray(e64, np.float64).reshape(-1)
    e = e[np.isfinite(e)]
    t = np.asarray(t, np.float64)
    lo = np.concatenate([(e[None] <= t[:, None] - band).sum(1), [len(e)]])
    hi = np.concatenate([(e[None] <= t[:, None] + band).sum(1), [len(e)]])
    out = (np.abs(e[None] - t[:, None]) < band).any(0).mean() if len(e) else 0.0
    return lo, hi, out


def check_counts(got, e64, t, what):
    lo, hi, out = bracket(e64, t)
    print('%s: %.3f %% of the values lie within %.1e m of a threshold' % (what, 100 * out, BAND))
    assert out <= 0.01, what
    assert (lo <= got).all() and (got <= hi).all(), what
    ref = R.threshold_counts(e64, t)
    same = lo == hi
    assert np.array_equal(got[same], ref[same]), what


def test_threshold_counts(pairs, refs):
    pd, gt = pairs
    t64 = AL.default_thresholds()
    thr = dev(t64)
    # the device's own errors against the restatement's float64 errors
    for name, idx in (('778', slice(None)), ('21', SUB)):
        err = AL.procrustes_align(dev(pd[:, idx]), dev(gt[:, idx]))['err']
        got = AL.threshold_counts(err, thr).cpu().numpy()
        e64 = np.array([r['err'] for r in refs[name]])
        check_counts(got, e64, t64, 'N = ' + name)
        assert got[-1] == e64.size
    # the same float32 numbers on both sides: every comparison is exact
    g = np.random.default_rng(9)
    e = np.abs(g.normal(0, 0.02, 200001)).astype(np.float32)
    e[::1000] = np.nan
    e[5::5000] = np.inf
    e[7] = -np.inf
    t32 = t64.astype(np.float32)
    ref = R.threshold_counts(e, t32)
    counts = AL.threshold_counts(dev(e), thr)
    assert np.array_equal(counts.cpu().numpy(), ref) and ref[-1] == np.isfinite(e).sum() < e.size          # NaNs are not examined
    again = AL.threshold_counts(dev(e), thr, counts)                                                     # a second call accumulates
    assert again is counts and np.array_equal(counts.cpu().numpy(), 2 * ref)
    few = AL.threshold_counts(dev(e[:3]), dev([0.5, 0.0, 0.01])).cpu().numpy()                           # any order, any K
    assert np.array_equal(few, R.threshold_counts(e[:3], np.array([0.5, 0.0, 0.01], np.float32)))
    k1024 = np.sort(g.uniform(0, 0.08, 1024)).astype(np.float32)
    assert np.array_equal(AL.threshold_counts(dev(e), dev(k1024)).cpu().numpy(), R.threshold_counts(e, k1024))
    with pytest.raises(ValueError):
        AL.threshold_counts(dev(e), thr, torch.zeros(101, dtype=torch.int32, device='cuda'))


def test_wrappers_check_their_arguments(pairs):
    from dir_amd import _capi
    pd, gt = pairs
    P, G = dev(pd[:4]), dev(gt[:4])
    with pytest.raises(_capi.DirHipError):
        AL.procrustes_align(P.cpu(), G)
    with pytest.raises(ValueError):
        AL.procrustes_align(P, G[:, :700])
    with pytest.raises(ValueError):
        AL.procrustes_align(P[:3], G)
    with pytest.raises(_capi.DirHipError):
        AL.procrustes_align(P[:, :2], G[:, :2])
    with pytest.raises(_capi.DirHipError):
        AL.nn_distances(torch.zeros(1, 4097, 3, device='cuda'), G[:1])
    with pytest.raises(_capi.DirHipError):
        AL.threshold_counts(P, torch.zeros(1025, device='cuda'))


# ------------------------------------------------------------------------------------------------------------------------ accumulator
@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def test_aligned_metrics_reproduce_the_restatement(state):
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import eval as EV
    mano = DS.gt_layers_from_checkpoint(state)
    jreg = {s: EV.Jr(mano[s].J_regressor) for s in ('left', 'right')}
    n = 48
    verts = {'left': R.pairs(n, seed=21), 'right': R.pairs(n, seed=22)}
    verts['left'][0][3, 100, 0] = np.nan                                     # one left hand without an alignment
    g = np.random.default_rng(4)
    offset = g.normal(0, 0.3, (n, 3)).astype(np.float32)
    v2d = {s: g.uniform(0, 256, (n, 778, 2)).astype(np.float32) for s in ('left', 'right')}
    cam = np.tile(np.array([[1500.0, 0, 128], [0, 1500.0, 128], [0, 0, 1]], np.float32), (n, 1, 1))
    m = AL.AlignedMetrics(jreg)
    joint_err = []
    for sl in (slice(0, 29), slice(29, 48)):                                  # two batches of different sizes
        result = [None, None, {'pd_mesh_xyz_left': dev(verts['left'][0][sl]), 'pd_mesh_xyz_right': dev(verts['right'][0][sl]),
                               'pd_offset': dev(offset[sl])}]
        data = (None, None, None, dev(verts['left'][1][sl]), None, dev(verts['right'][1][sl]), None, dev(v2d['left'][sl]), None,
                dev(v2d['right'][sl]), dev(cam[sl]))
        m.update(result, data)
        out = EV.eval_batch(jreg, {'left': result[2]['pd_mesh_xyz_left'], 'right': result[2]['pd_mesh_xyz_right']}, result[2]['pd_offset'],
                            {'left': data[3], 'right': data[5]}, {'left': data[7], 'right': data[9]}, data[10])
        joint_err.append(out['joint_err'].cpu().numpy())
    joint_err = np.concatenate(joint_err)
    torch.cuda.synchronize()
    s, a = m.summarize(), m.arrays()
    assert s['invalid'] == {'left': 1, 'right': 0} and s['samples'] == {'left': n - 1, 'right': n}
    t = m.thresholds
    for h, side in enumerate(('left', 'right')):
        J = jreg[side].J_regressor.cpu().numpy().astype(np.float64)
        pd, gt = verts[side][0].astype(np.float64), verts[side][1].astype(np.float64)
        valid = a[side]['valid']
        assert valid.sum() == s['samples'][side]
        ref = R.summary(J @ pd, J @ gt, pd, gt, joint_err[valid, h], t)
        ej, ev = a[side]['err_joint'][valid].astype(np.float64), a[side]['err_vert'][valid].astype(np.float64)
        dj, dv = np.abs(ej - ref['err_joint']).max(), np.abs(ev - ref['err_vert']).max()
        print('%s: max |PA joint err - ref| = %.3e m, max |PA vertex err - ref| = %.3e m' % (side, dj, dv))
        assert dj < POS_GATE and dv < POS_GATE
        assert abs(s['pa_mpjpe_mm'][side] - ref['pa_mpjpe_mm']) < POS_GATE * 1000 and abs(s['pa_mpvpe_mm'][side] - ref['pa_mpvpe_mm']) < POS_GATE * 1000
        # the unaligned curve counts eval_batch's own float32 errors (the root joint's is exactly 0, which is also the first threshold): the
        # same float32 numbers are on both sides, so every comparison with the float32 thresholds is exact and no band is needed
        t32 = t.astype(np.float32)
        cu = R.threshold_counts(joint_err[valid, h], t32)
        assert np.array_equal(a['counts'][h, 2], cu) and cu[-1] == 21 * valid.sum()
        assert s['auc_joint'][side] == R.auc(cu, t) and np.array_equal(s['pck_joint'][side], R.pck(cu))
        for c, (name, e64) in enumerate((('pa_joint', ref['err_joint']), ('pa_vert', ref['err_vert']))):
            check_counts(a['counts'][h, c], e64, t, '%s %s' % (side, name))
            lo, hi, _ = bracket(e64, t)
            if np.array_equal(lo, hi):
                assert s['auc_' + name][side] == ref['auc_' + name] and np.array_equal(s['pck_' + name][side], R.pck(ref['counts_' + name]))
            assert R.auc(lo, t) <= s['auc_' + name][side] <= R.auc(hi, t)
        # F-scores: exact for the samples none of whose distances lies within the band of tau; the others between the scores with every
        # such distance counted out and counted in (F grows with both shares)
        f = m.f_scores(side)[valid]
        d_all = np.concatenate([ref['d_pd'], ref['d_gt']], 1)
        for k, tau in enumerate(R.F_TAUS):
            near = (np.abs(d_all - tau) < BAND)
            print('%s F@%g mm: %.3f %% of the distances lie within the band, %d of %d samples have none' % (side, tau * 1000, 100 * near.mean(), (~near.any(1)).sum(), len(near)))
            assert near.mean() <= 0.01
            want = np.array([R.f_score(x, y, tau) for x, y in zip(ref['d_pd'], ref['d_gt'])])
            lo = np.array([R.f_score(x, y, tau - BAND) for x, y in zip(ref['d_pd'], ref['d_gt'])])
            hi = np.array([R.f_score(x, y, tau + BAND) for x, y in zip(ref['d_pd'], ref['d_gt'])])
            clear = ~near.any(1)
            assert clear.any() and np.array_equal(f[clear, k], want[clear]), (side, tau)
            assert (lo <= f[:, k]).all() and (f[:, k] <= hi).all(), (side, tau)
            assert lo.mean() - 1e-15 <= s['f_%d' % round(tau * 1000)][side] <= hi.mean() + 1e-15
            if clear.all():
                assert abs(s['f_%d' % round(tau * 1000)][side] - ref['f_%d' % round(tau * 1000)]) < 1e-15
        assert 0 < s['f_5'][side] < s['f_15'][side] <= 1
    for k in ('pa_mpjpe_mm', 'auc_pa_joint', 'f_5'):
        assert s[k]['all'] == (s[k]['left'] + s[k]['right']) / 2
    text = m.report()
    assert 'PA-MPJPE' in text and 'F@15 mm' in text and 'hands left out' in text and 'left 1, right 0' in text


# ------------------------------------------------------------------------------------------------------------------------ wiring
TWELVE = sorted(['left_joint.txt', 'right_joint.txt', 'joint_left_error.txt', 'joint_right_error.txt', 'mesh_left_error.txt',
                 'mesh_right_error.txt', 'joint_2d_left_error.txt', 'joint_2d_right_error.txt', 'mesh_2d_left_error.txt',
                 'mesh_2d_right_error.txt', 'root_loss.txt', 'volume.txt'])
NEW = sorted(['pa_joint_left_error.txt', 'pa_joint_right_error.txt', 'pa_mesh_left_error.txt', 'pa_mesh_right_error.txt', 'fscore.txt', 'pck.txt'])


def test_eval_command_line_with_and_without_aligned(tmp_path, state, capsys):
    from dir_amd.apps import eval as EV
    n = 20
    write_split(str(tmp_path / 'data'), n, seed=5)
    ck = tmp_path / 'DIR.pth'
    torch.save({'net': state, 'last_epoch': 0}, str(ck))
    args = ['--model', str(ck), '--data_path', str(tmp_path / 'data'), '--workers', '2', '--dtype', 'bf16']
    plain = EV.main(args + ['--bs', '4', '--result_dir', str(tmp_path / 'plain')])
    text_plain = capsys.readouterr().out
    m4 = EV.main(args + ['--bs', '4', '--result_dir', str(tmp_path / 'a4'), '--aligned'])
    text4 = capsys.readouterr().out
    EV.main(args + ['--bs', '16', '--result_dir', str(tmp_path / 'a16'), '--aligned'])
    capsys.readouterr()
    # without the flag: the twelve files and the report as they were, nothing new
    assert sorted(os.listdir(tmp_path / 'plain')) == TWELVE and 'aligned' not in text_plain and 'PA-' not in text_plain
    assert not hasattr(plain, 'aligned')
    assert plain.report() + '\n' in text_plain and 'images/s from files' in text_plain.split(plain.report() + '\n')[1].splitlines()[0]
    assert sorted(os.listdir(tmp_path / 'a4')) == sorted(TWELVE + NEW) == sorted(os.listdir(tmp_path / 'a16'))
    for name in TWELVE:
        assert open(tmp_path / 'plain' / name, 'rb').read() == open(tmp_path / 'a4' / name, 'rb').read(), name
    for name in NEW:
        assert open(tmp_path / 'a4' / name, 'rb').read() == open(tmp_path / 'a16' / name, 'rb').read(), name          # any batch size
    # the block comes after the reference's lines, before the rate
    head, tail = text4.split(m4.report() + '\n')
    assert 'aligned' not in head and 'images/s from files' in tail.splitlines()[-1]
    block = '\n'.join(tail.splitlines()[:-1])
    assert block == m4.aligned.report() and block.startswith('aligned') and all(w in block for w in ('PA-MPJPE', 'PA-MPVPE', 'AUC', 'F@5 mm', 'F@15 mm'))
    # the files hold what the accumulator holds
    a, s = m4.aligned.arrays(), m4.aligned.summarize()
    pj = np.loadtxt(str(tmp_path / 'a4' / 'pa_joint_left_error.txt'))
    pm = np.loadtxt(str(tmp_path / 'a4' / 'pa_mesh_right_error.txt'))
    fs, pck = np.loadtxt(str(tmp_path / 'a4' / 'fscore.txt')), np.loadtxt(str(tmp_path / 'a4' / 'pck.txt'))
    assert pj.shape == (n, 21) and pm.shape == (n,) and fs.shape == (n, 4) and pck.shape == (100, 7)
    assert np.abs(pj - a['left']['err_joint'] * 1000).max() < 6e-4 and np.abs(pm - a['right']['err_vert'].mean(-1) * 1000).max() < 6e-4
    assert abs(pj.mean() - s['pa_mpjpe_mm']['left']) < 6e-4 and np.abs(pck[:, 0] - np.linspace(0, 50, 100)).max() < 1e-6
    assert (np.diff(pck[:, 1:], axis=0) >= 0).all() and (pck[:, 1:] >= 0).all() and (pck[:, 1:] <= 1).all()
    assert s['invalid'] == {'left': 0, 'right': 0} and s['samples'] == {'left': n, 'right': n}
    assert 0 < s['pa_mpjpe_mm']['all'] and 0 <= s['f_5']['all'] <= s['f_15']['all'] <= 1


def test_validate_reports_aligned_errors(tmp_path, state):
    from fake_train_split import write_train_split
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import train as T
    from dir_amd.apps.trainset import TrainBatches
    from dir_amd.models.dir import DIR
    d = str(tmp_path / 'split')
    write_train_split(d, 8, seed=11)
    shutil.copytree(os.path.join(d, 'train'), os.path.join(d, 'test'))
    mano = DS.gt_layers_from_checkpoint(state)
    model = DIR(21, 'unused', 0, compute_dtype=torch.float16)
    model.load_state_dict(state, strict=True)
    model.autotune = False
    model = model.cuda()
    vb = lambda: TrainBatches(d, mano, 'test', batch_size=4, workers=2, seed=3, augment=False, shuffle=False)  # noqa: E731
    before = T.validate(model, vb(), quiet=True)

    class Log:
        lines = []

        def info(self, l):
            self.lines.append(l)
    res = T.validate(model, vb(), quiet=True, aligned=True, logger=Log())
    assert sorted(set(res) - set(before)) == ['PA_MPJPE_2', 'PA_MPVPE_2']
    assert all(res[k] == before[k] for k in before)                          # 'error' (which selects best.pth) included
    for k in ('PA_MPJPE_2', 'PA_MPVPE_2'):
        assert sorted(res[k]) == ['all', 'left', 'right'] and all(np.isfinite(v) and v > 0 for v in res[k].values())
        assert res[k]['all'] == (res[k]['left'] + res[k]['right']) / 2
    assert sum('PA_MPJPE_2' in l and 'PA_MPVPE_2' in l for l in Log.lines) == 1
    assert T.build_parser().parse_args(['--init', 'x', '--eval_aligned']).eval_aligned
