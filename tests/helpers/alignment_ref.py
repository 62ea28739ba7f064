"""float64 numpy restatement of the aligned evaluation measures (dir_amd/csrc/alignmetric.hip and dir_amd/utils/alignment.py state the
same rules), and the point sets the tests put through both.  Nothing here is shared with the product code.

  procrustes        the similarity (s, R, t) that maps pd onto gt in the least-squares sense (Umeyama 1991): np.linalg.svd of the
                    covariance with the det fix, so R is always a proper rotation; -> dict(s, R, t, aligned, err, sigma, det_fix)
  nn                brute-force nearest-neighbour distances both ways, point to point
  threshold_counts  counts[k] = number of finite err <= thresholds[k]; counts[K] = number of finite err
  pck / auc         counts -> the PCK curve; trapz(PCK, t) / (t[-1] - t[0])
  f_score           F = 2PR / (P + R) from the two distance sets at one threshold (0 when P + R = 0)
  summary           what utils.alignment.AlignedMetrics.summarize() reports, from raw predicted / ground-truth vertices
  random_rotation, pairs      the seeded inputs of the GPU tests
"""
import numpy as np

THRESHOLDS = np.linspace(0, 0.05, 100)
F_TAUS = (0.005, 0.015)


def procrustes(pd, gt, scale=True):
    pd, gt = np.asarray(pd, np.float64), np.asarray(gt, np.float64)
    mp, mg = pd[0] + (pd - pd[0]).mean(0), gt[0] + (gt - gt[0]).mean(0)      # about the first point: equal points give exactly 0 below
    p, g = pd - mp, gt - mg
    var = (p * p).sum()
    nan = dict(s=np.nan, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), aligned=np.full_like(pd, np.nan), err=np.full(len(pd), np.nan),
               sigma=np.full(3, np.nan), det_fix=False)
    if not (np.isfinite(pd).all() and np.isfinite(gt).all()) or var == 0:
        return nan
    H = g.T @ p                                        # sum_i g_i p_i^T: maximise trace(R^T H) = sum_i g_i . R p_i
    U, sig, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    D = np.diag([1.0, 1.0, d if d != 0 else 1.0])
    R = U @ D @ Vt
    s = (sig * np.diag(D)).sum() / var if scale else 1.0
    t = mg - s * R @ mp
    aligned = s * pd @ R.T + t
    return dict(s=s, R=R, t=t, aligned=aligned, err=np.linalg.norm(aligned - gt, axis=1), sigma=sig, det_fix=bool(d < 0))


def well_posed(ref):
    """the gap that makes the maximiser unique, relative to sigma_1: sigma_2 without the det fix, sigma_2 - sigma_3 with it"""
    s = ref['sigma']
    return (s[1] - s[2]) / s[0] if ref['det_fix'] else s[1] / s[0]


def nn(a, b):
    """-> (d_ab [Na], d_ba [Nb])"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1))
    return d.min(1), d.min(0)


def threshold_counts(err, thresholds):
    e, t = np.asarray(err, np.float64).reshape(-1), np.asarray(thresholds, np.float64)
    e = e[np.isfinite(e)]
    return np.concatenate([(e[None] <= t[:, None]).sum(1), [len(e)]]).astype(np.int64)


def pck(counts):
    c = np.asarray(counts, np.float64)
    return c[:-1] / c[-1] if c[-1] else np.full(len(c) - 1, np.nan)


def auc(counts, thresholds):
    t = np.asarray(thresholds, np.float64)
    y = pck(counts)
    return float(((y[1:] + y[:-1]) / 2 * np.diff(t)).sum() / (t[-1] - t[0]))


def f_score(d_pd, d_gt, tau):
    """d_pd: predicted points to the nearest ground-truth point; d_gt: the reverse"""
    P, R = (np.asarray(d_pd) < tau).mean(), (np.asarray(d_gt) < tau).mean()
    return float(2 * P * R / (P + R)) if P + R > 0 else 0.0


def summary(joints_pd, joints_gt, verts_pd, verts_gt, joint_err=None, thresholds=THRESHOLDS):
    """One hand: joints [n,21,3], vertices [n,V,3] (raw prediction and ground truth), joint_err [n,21] the root-relative unaligned joint
    errors -> the numbers AlignedMetrics.summarize() gives for that hand, plus the per-sample arrays behind them"""
    n = len(joints_pd)
    ej, ev, dp, dg = [], [], [], []
    for i in range(n):
        rj, rv = procrustes(joints_pd[i], joints_gt[i]), procrustes(verts_pd[i], verts_gt[i])
        if np.isnan(rj['s']) or np.isnan(rv['s']):
            continue
        ej.append(rj['err'])
        ev.append(rv['err'])
        a, b = nn(rv['aligned'], verts_gt[i])
        dp.append(a)
        dg.append(b)
    ej, ev = np.array(ej).reshape(-1, joints_pd.shape[1]), np.array(ev).reshape(-1, verts_pd.shape[1])
    cj, cv = threshold_counts(ej, thresholds), threshold_counts(ev, thresholds)
    out = {'samples': len(ej), 'invalid': n - len(ej), 'pa_mpjpe_mm': float(ej.mean() * 1000), 'pa_mpvpe_mm': float(ev.mean() * 1000),
           'counts_pa_joint': cj, 'counts_pa_vert': cv, 'auc_pa_joint': auc(cj, thresholds), 'auc_pa_vert': auc(cv, thresholds),
           'err_joint': ej, 'err_vert': ev, 'd_pd': np.array(dp), 'd_gt': np.array(dg)}
    for tau in F_TAUS:
        out['f_%d' % round(tau * 1000)] = float(np.mean([f_score(a, b, tau) for a, b in zip(dp, dg)]))
    if joint_err is not None:
        out['counts_joint'] = threshold_counts(joint_err, thresholds)
        out['auc_joint'] = auc(out['counts_joint'], thresholds)
    return out


def random_rotation(g):
    """a proper rotation, uniformly distributed: QR of a Gaussian matrix, signs fixed"""
    q, r = np.linalg.qr(g.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pairs(n=64, seed=0, gt_noise=0.003, pd_noise=0.008):
    """the GPU tests' inputs: gt = the synthetic right template + 3 mm noise; pd = s Q (gt + 8 mm noise) + t with a random rotation Q,
    s in 0.7 .. 1.3 and |t| about 0.1 m; every eighth pair mirrored in x.  -> (pd float32 [n,778,3], gt float32 [n,778,3])"""
    from dir_amd import synth
    tpl = np.asarray(synth.synthetic_mano_tables('right')['v_template'], np.float64)
    g = np.random.default_rng(seed)
    pd, gt = np.empty((n,) + tpl.shape), np.empty((n,) + tpl.shape)
    for i in range(n):
        gt[i] = tpl + g.normal(0, gt_noise, tpl.shape)
        x = gt[i] + g.normal(0, pd_noise, tpl.shape)
        if i % 8 == 7:
            x = x * np.array([-1.0, 1.0, 1.0])
        d = g.normal(size=3)
        pd[i] = g.uniform(0.7, 1.3) * x @ random_rotation(g).T + 0.1 * d / np.linalg.norm(d) * g.uniform(0.8, 1.2)
    return pd.astype(np.float32), gt.astype(np.float32)


SUBSET21 = tuple(int(i) for i in np.linspace(0, 777, 21).round())


def planar_mirror(n=40, seed=3):
    """a planar set (in the plane through the origin with normal (1, 2, 2) / 3, shifted) and its in-plane mirror image -> (pd, gt, axis):
    gt is pd mirrored in the in-plane line along `axis`, which the flip about that axis (a proper rotation by pi) reproduces exactly"""
    g = np.random.default_rng(seed)
    nrm = np.array([1.0, 2.0, 2.0]) / 3
    u = np.cross(nrm, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    w = np.cross(nrm, u)
    c = g.uniform(-0.08, 0.08, (n, 2)) * [1.0, 0.6]
    pd = c[:, :1] * u + c[:, 1:] * w
    gt = c[:, :1] * u - c[:, 1:] * w                       # mirrored in the line along u
    return pd + [0.02, -0.01, 0.4], gt + [-0.1, 0.03, 0.5], u
