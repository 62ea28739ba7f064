"""Measures the pair fit (dir_mano_fit_pair, utils/mano_fit.py fit_mano_pair) on the GPU.  No gates: it prints what it finds.

  python tools/bench_mano_pair_fit.py [--b 32 256] [--rounds 20] [--iters 50]
      HIP events, one process, warmed, the variants alternating round by round; median and range per variant.  B pairs = 2 x B hands: random hands
      a few centimetres apart (their 8 mm capsules overlap), 3-D joint targets generated from the same parameters, started from them + noise, as
        single_N       dir_mano_fit on the 2 x B hands (grid B x 2, 256 threads): no coupling exists
        pair_off_N     dir_mano_fit_pair with w_col = 0, lr_o = 0: the 512-thread pair workgroup and its extra barriers, no capsule phase
        pair_on_N      dir_mano_fit_pair with w_col = 1e4 and the offset moving: the capsule phase, the gather and the fifth Adam group every iteration
        fwd_bwd        one dir_mano_forward_pair + one dir_mano_backward_pair: the floor of an iteration built from the two kernels
      Reported: microseconds per call and per iteration, and what the pair workgroup and the collision phase add to dir_mano_fit's iteration.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def measure(B, N, rounds):
    import torch

    from dir_amd import functional as F
    from dir_amd.engine import run_mano_pair
    from dir_amd.manopth.manolayer import ManoLayer
    from dir_amd.utils import mano_fit as MF
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=9, flat_hand_mean=False, side=s).cuda() for s in ('left', 'right')]
    tabs = [m.c_tables(9) for m in layers]
    rng = np.random.default_rng(0)
    truth, start = [], []
    for _ in range(2):
        p = MF.neutral_para(B, 4.0)
        p[:, :6] += torch.from_numpy(rng.normal(0, 0.2, (B, 6)).astype(np.float32)).cuda()
        p[:, 6:61] = torch.from_numpy(rng.normal(0, 0.4, (B, 55)).astype(np.float32)).cuda()
        truth.append(p)
        q = p.clone()
        q[:, :51] += torch.from_numpy(rng.normal(0, 0.05, (B, 51)).astype(np.float32)).cuda()
        start.append(q)
    (_, jl, _), (_, jr, _) = run_mano_pair(tabs, truth[0], truth[1], B)
    targets = [jl.clone(), jr.clone()]
    o0 = torch.from_numpy(rng.normal(0, 0.015, (B, 3)).astype(np.float32)).cuda()
    radii = [torch.full((20,), 0.008, device='cuda'), torch.full((20,), 0.008, device='cuda')]
    W, LR = {'w_joints': 1e4, 'w_init': 1e-2}, [0.01, 0.01, 0.0, 0.01]

    def single():
        return F.mano_fit(tabs, start, joints=targets, iters=N, lr=LR, weights=W)

    def pair(w_col, lr_o):
        return lambda: F.mano_fit_pair(tabs, start, o0, radii, joints=targets, iters=N, lr=LR, lr_offset=lr_o, weights=W,
                                       pair_weights={'w_col': w_col, 'w_off_init': 1.0 if w_col else 0.0})

    def fwd_bwd():
        (vl, _, _), (vr, _, _) = run_mano_pair(tabs, start[0], start[1], B)
        F.mano_backward(tabs, start, g_verts=[vl, vr])
    variants = {'single_%d' % N: (single, N), 'pair_off_%d' % N: (pair(0.0, 0.0), N), 'pair_on_%d' % N: (pair(1e4, 3e-3), N), 'fwd_bwd': (fwd_bwd, 1)}
    for fn, _ in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, (b, _), (_, c) = single(), pair(0.0, 0.0)(), pair(1e4, 3e-3)()
    torch.cuda.synchronize()
    same = all(torch.equal(x['para'].view(torch.int32), y['para'].view(torch.int32)) for x, y in zip(a, b))
    col = c['col'].cpu().numpy()
    print('B = %d pairs: pair_off gives dir_mano_fit\'s parameters bit for bit: %s; pair_on: %d of %d pairs overlap at the start, largest overlap %.2f -> %.2f mm' % (
        B, same, int((col[:, 1] > 0).sum()), B, col[:, 1].max() * 1e3, col[:, 3].max() * 1e3))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, _) in variants.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0)
    res = {}
    for k, (_, n) in variants.items():
        t = np.array(times[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max()), 'us_per_iteration': float(np.median(t)) / n}
        print('%-14s %10.1f us  (%.1f .. %.1f)  %8.1f us per iteration' % (k, res[k]['us_median'], t.min(), t.max(), res[k]['us_per_iteration']))
    s, off, on = (res[k % N]['us_per_iteration'] for k in ('single_%d', 'pair_off_%d', 'pair_on_%d'))
    print('per iteration: the pair workgroup adds %.1f us to dir_mano_fit (x %.2f), the collision phase %.1f us more (x %.2f); single / (forward + backward) = %.2f' % (
        off - s, off / s, on - off, on / off, s / res['fwd_bwd']['us_median']))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--b', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=50)
    opt = ap.parse_args()
    out = {}
    for B in opt.b:
        out['B%d' % B] = measure(B, opt.iters, opt.rounds)
    print(json.dumps({'bench_mano_pair_fit': out}))


if __name__ == '__main__':
    main()
