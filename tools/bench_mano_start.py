"""Measures the closed-form start of a MANO fit (dir_mano_fit_start, utils/mano_fit.py start_mano) on the GPU.  No gates: it prints what it finds.

  python tools/bench_mano_start.py [--b 32 256] [--rounds 20] [--calls 20] [--iters 50]
      HIP events around `calls` back-to-back calls, one process, warmed, the variants alternating round by round; median and range per variant,
      microseconds per call.  B x 2 hands, targets generated from random parameters whose root is rotated by 1.8 .. 3.1 rad, cold start, as
        forward          dir_mano_forward_pair at the start: the forward that the start launch contains
        start_mesh       dir_mano_fit_start on mesh targets (two reductions over the vertices, Horn's rotation)
        start_all        the same with 3-D joints and 2-D keypoints as well (+ the camera)
        start_uv         2-D keypoints alone (the search over the cube's 24 rotations, one camera each)
        fit_N            fit_mano, N iterations, mesh targets, from the cold start
        fit_N_closed     fit_mano(start='closed'): the start launch, then the same fit
      Reported: the ratios start / forward and fit_N_closed / fit_N, and the worst vertex RMS of the two fits.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def bench(B, opt):
    import torch

    from dir_amd import functional as F
    from dir_amd.engine import run_mano_pair
    from dir_amd.manopth.manolayer import ManoLayer
    from dir_amd.utils import mano_fit as MF
    N = opt.iters
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=9, flat_hand_mean=False, side=s).cuda() for s in ('left', 'right')]
    tabs = [m.c_tables(9) for m in layers]
    rng = np.random.default_rng(0)
    truth = []
    for _ in range(2):
        p = np.zeros((B, 64), np.float32)
        for i in range(B):
            ax, ang = rng.normal(0, 1, 3), rng.uniform(1.8, 3.1)
            ax /= np.linalg.norm(ax)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            rot = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
            p[i, 0:3], p[i, 3:6] = rot[:, 0], rot[:, 1]
        p[:, 6:51] = rng.normal(0, 0.4, (B, 45))
        p[:, 51:61] = rng.normal(0, 0.5, (B, 10))
        p[:, 61] = rng.uniform(3.5, 4.5, B)
        truth.append(torch.from_numpy(p).cuda())
    (vl, jl, ul), (vr, jr, ur) = run_mano_pair(tabs, truth[0], truth[1], B)
    V, J, U = [vl, vr], [jl, jr], [ul, ur]
    cold = [MF.neutral_para(B, 4.0), MF.neutral_para(B, 4.0)]
    W = {'w_verts': 1e4}
    variants = {
        'forward': lambda: run_mano_pair(tabs, cold[0], cold[1], B),
        'start_mesh': lambda: F.mano_fit_start(tabs, cold, verts=V, w_verts=1e4),
        'start_all': lambda: F.mano_fit_start(tabs, cold, verts=V, joints=J, joint_uv=U, w_verts=1e4, w_joints=1e4),
        'start_uv': lambda: F.mano_fit_start(tabs, cold, joint_uv=U),
        'fit_%d' % N: lambda: MF.fit_mano(tabs, cold, verts=V, iters=N, lr=0.1, weights=W, outputs=False),
        'fit_%d_closed' % N: lambda: MF.fit_mano(tabs, cold, verts=V, iters=N, lr=0.1, weights=W, outputs=False, start='closed'),
    }
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, b = variants['fit_%d' % N](), variants['fit_%d_closed' % N]()
    st = F.mano_fit_start(tabs, cold, joint_uv=U)
    torch.cuda.synchronize()
    rms = lambda r: float(torch.stack(r.mse_after)[:, :, 0].sqrt().max()) * 1e3  # noqa: E731
    print('B = %d x 2 hands: worst vertex RMS after %d iterations %.3f mm cold, %.3f mm started; 2-D search: %d of %d rows wrote a rotation' % (
        B, N, rms(a), rms(b), sum(int((r['choice'] >= 0).sum()) for r in st), 2 * B))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, fn in variants.items():
            calls = opt.calls if not k.startswith('fit') else max(1, opt.calls // 10)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / calls)
    res = {}
    for k in variants:
        t = np.array(times[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max())}
        print('%-16s %10.1f us per call  (%.1f .. %.1f)' % (k, res[k]['us_median'], t.min(), t.max()))
    f = res['forward']['us_median']
    print('start / forward: mesh %.2f, all %.2f, uv %.2f;  fit_%d_closed / fit_%d = %.3f' % (
        res['start_mesh']['us_median'] / f, res['start_all']['us_median'] / f, res['start_uv']['us_median'] / f, N, N,
        res['fit_%d_closed' % N]['us_median'] / res['fit_%d' % N]['us_median']))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--b', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--iters', type=int, default=50)
    opt = ap.parse_args()
    print('%d rounds, %d back-to-back calls per round and variant (fits: %d), variants alternating' % (opt.rounds, opt.calls, max(1, opt.calls // 10)))
    print(json.dumps({'bench_mano_start': {str(B): bench(B, opt) for B in opt.b}}))


if __name__ == '__main__':
    main()
