"""CPU-only: the float64 restatement of the aligned evaluation measures (tests/helpers/alignment_ref.py) against closed forms, and the
host-side contract of the three C entry points (no launch: there is no GPU here)."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import alignment_ref as R  # noqa: E402

from test_capi_exports import declared_symbols  # noqa: E402

NAMES = ('dir_procrustes_align', 'dir_point_set_nn', 'dir_threshold_counts')


def cloud(n=50, seed=0):
    return np.random.default_rng(seed).normal(0, 0.05, (n, 3)) * [1.0, 0.6, 0.3]


def test_a_known_similarity_is_recovered_with_zero_error():
    g = np.random.default_rng(1)
    for k in range(5):
        x, Q, s, t = cloud(30 + k, k), R.random_rotation(g), g.uniform(0.5, 2), g.normal(0, 0.2, 3)
        gt = s * x @ Q.T + t
        r = R.procrustes(x, gt)
        assert abs(r['s'] - s) < 1e-13 and np.abs(r['R'] - Q).max() < 1e-13 and np.abs(r['t'] - t).max() < 1e-13
        assert r['err'].max() < 1e-15 and np.abs(r['aligned'] - gt).max() < 1e-15 and not r['det_fix']


def test_a_mirrored_set_gets_a_proper_rotation_and_a_non_zero_error():
    x = cloud(40, 2)
    gt = x * [-1.0, 1.0, 1.0] + [0.1, 0, 0]
    r = R.procrustes(x, gt)
    assert r['det_fix'] and abs(np.linalg.det(r['R']) - 1) < 1e-13 and np.abs(r['R'] @ r['R'].T - np.eye(3)).max() < 1e-13
    assert r['err'].mean() > 0.005 and 0 < r['s'] < 1
    # no proper rotation does better: the fit's sum of squares is below that of 200 random ones with their own best scale (a negative
    # scale would be a reflection again, so it is held at 0)
    g, p, q = np.random.default_rng(3), x - x.mean(0), gt - gt.mean(0)
    for _ in range(200):
        Q = R.random_rotation(g)
        s = max(0.0, (q * (p @ Q.T)).sum() / (p * p).sum())
        assert ((s * p @ Q.T - q) ** 2).sum() >= (r['err'] ** 2).sum() - 1e-15


def test_a_planar_set_and_its_in_plane_mirror_image_align_exactly_by_a_flip():
    pd, gt, axis = R.planar_mirror()
    r = R.procrustes(pd, gt)
    assert r['err'].max() < 1e-15 and abs(r['s'] - 1) < 1e-13
    assert abs(np.linalg.det(r['R']) - 1) < 1e-13 and abs(np.trace(r['R']) + 1) < 1e-13          # a rotation by pi
    assert np.abs(r['R'] @ axis - axis).max() < 1e-13                                          # about the in-plane axis


def test_scale_off_gives_one():
    x = cloud(25, 4)
    Q = R.random_rotation(np.random.default_rng(5))
    gt = 1.7 * x @ Q.T + [0.3, 0.1, -0.2]
    r = R.procrustes(x, gt, scale=False)
    assert r['s'] == 1.0 and np.abs(r['R'] - Q).max() < 1e-13 and r['err'].max() > 0.01
    assert np.abs(r['aligned'] - (x @ r['R'].T + r['t'])).max() < 1e-16


def test_degenerate_input_gives_nan():
    x = cloud(10, 6)
    same = np.tile([[0.1, 0.2, 0.3]], (10, 1))
    assert np.isnan(R.procrustes(same, x)['err']).all() and np.isnan(R.procrustes(same, x)['s'])
    bad = x.copy()
    bad[3, 1] = np.nan
    assert np.isnan(R.procrustes(bad, x)['err']).all() and np.isnan(R.procrustes(x, bad)['aligned']).all()
    line = np.linspace(0, 1, 10)[:, None] * [[1.0, 2.0, -1.0]]
    r = R.procrustes(line, x)                                        # collinear: some maximiser, finite and proper
    assert np.isfinite(r['aligned']).all() and abs(np.linalg.det(r['R']) - 1) < 1e-12


def test_counts_pck_and_auc():
    t = R.THRESHOLDS
    assert len(t) == 100 and t[0] == 0 and abs(t[-1] - 0.05) < 1e-18
    zeros = R.threshold_counts(np.zeros(30), t)
    assert (zeros == 30).all() and R.auc(zeros, t) == 1.0
    far = R.threshold_counts(np.full(30, 0.0501), t)
    assert (far[:-1] == 0).all() and far[-1] == 30 and R.auc(far, t) == 0.0
    e = np.array([0.0, 0.01, 0.025, np.nan, 0.06, np.inf])
    c = R.threshold_counts(e, t)
    assert c[-1] == 4 and c[0] == 1 and c[99] == 3 and c[50] == (e[np.isfinite(e)] <= t[50]).sum()
    # a uniform error distribution over 0..50 mm: PCK(t) = t / 50 mm, AUC = 1/2
    u = R.threshold_counts((np.arange(100000) + 0.5) / 100000 * 0.05, t)
    assert abs(R.auc(u, t) - 0.5) < 1e-4 and np.abs(R.pck(u) - t / 0.05).max() < 1e-4


def test_f_scores():
    a = cloud(60, 7)
    d1, d2 = R.nn(a, a)
    assert (d1 == 0).all() and (d2 == 0).all() and R.f_score(d1, d2, 0.005) == 1.0
    b = a + [1.0, 0, 0]                                              # more than tau apart
    d1, d2 = R.nn(a, b)
    assert d1.min() > 0.5 and R.f_score(d1, d2, 0.005) == 0.0 and R.f_score(d1, d2, 0.015) == 0.0
    # half of the predicted points on the ground truth, half far away, every ground-truth point covered: P = 1/2, R = 1, F = 2/3
    pd = np.concatenate([a, a + [1.0, 0, 0]])
    d_pd, d_gt = R.nn(pd, a)
    assert abs(R.f_score(d_pd, d_gt, 0.005) - 2 / 3) < 1e-15
    # nn against brute force with different sizes
    c = cloud(17, 8)
    d_ac, d_ca = R.nn(a, c)
    assert d_ac.shape == (60,) and d_ca.shape == (17,)
    assert d_ac[5] == min(np.linalg.norm(a[5] - x) for x in c) and d_ca[3] == min(np.linalg.norm(c[3] - x) for x in a)


def test_the_gpu_tests_pairs_are_well_posed():
    pd, gt = R.pairs(64)
    gaps = []
    for i in range(64):
        for idx in (slice(None), list(R.SUBSET21)):
            r = R.procrustes(pd[i][idx], gt[i][idx])
            assert r['det_fix'] == (i % 8 == 7)
            gaps.append(R.well_posed(r))
    print('smallest gap: %.3f' % min(gaps))
    assert min(gaps) >= 1e-2


def test_binding_holds_the_three_entry_points():
    from dir_amd import _capi
    syms = declared_symbols()
    for n in NAMES:
        assert n in _capi._SIGNATURES and n in syms
    assert sorted(_capi._SIGNATURES) == syms


def test_entry_points_reject_bad_arguments_before_any_launch():
    import torch  # noqa: F401
    from dir_amd import _capi, build
    build.build(verbose=False)
    L = _capi.lib()
    assert L.dir_abi_version() == _capi.ABI_VERSION
    one = ctypes.c_void_p(16)

    def bad(rc, word):
        assert rc != 0 and word in L.dir_last_error(), (rc, L.dir_last_error())

    def fit(pd=one, gt=one, B=2, N=778, flags=1, err=one):
        return L.dir_procrustes_align(pd, gt, B, N, flags, None, None, err, None)

    def nn(a=one, b=one, B=2, Na=778, Nb=778, dab=one, dba=one):
        return L.dir_point_set_nn(a, b, B, Na, Nb, dab, dba, None)

    def cnt(err=one, n=100, thr=one, K=100, counts=one):
        return L.dir_threshold_counts(err, n, thr, K, counts, None)
    for k in ('pd', 'gt', 'err'):
        bad(fit(**{k: None}), b'null pointer')
    bad(fit(B=0), b'batch')
    bad(fit(B=-1), b'batch')
    bad(fit(N=2), b'points')
    bad(fit(N=4097), b'points')
    bad(fit(flags=2), b'flags')
    for k in ('a', 'b', 'dab', 'dba'):
        bad(nn(**{k: None}), b'null pointer')
    bad(nn(B=0), b'batch')
    bad(nn(Na=0), b'points')
    bad(nn(Nb=4097), b'points')
    for k in ('err', 'thr', 'counts'):
        bad(cnt(**{k: None}), b'null pointer')
    bad(cnt(n=0), b'values')
    bad(cnt(n=1 << 31), b'values')
    bad(cnt(K=0), b'thresholds')
    bad(cnt(K=1025), b'thresholds')
