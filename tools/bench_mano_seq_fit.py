"""Measures the sequence fit (dir_mano_fit_sequence, csrc/mano_fit_seq.hip) on the GPU.  No gates: it prints what it finds.

  python tools/bench_mano_seq_fit.py [--frames 64 512] [--seq 64] [--iters 50] [--rounds 20]
      HIP events, one process, warmed, the variants alternating round by round; median and range per variant.  N frames x 2 hands in sequences of
      --seq frames, 3-D joint targets generated from random smooth tracks, cold start, as
        seq_shared     dir_mano_fit_sequence, one shape per (sequence, hand), the three temporal weights 1: two launches per iteration
        seq_per_frame  the same with a shape per frame: one launch per iteration
        fit            dir_mano_fit on the same frames: the independent fit it contains, the loop inside ONE launch
        composed       the independent loop as a user of the older launches would write it: dir_mano_forward_pair, ATen residual operations,
                       F.mano_backward (dir_mano_backward_pair) and a foreach torch.optim.Adam, per iteration
      Reported: microseconds per call and per iteration, and beside them the HOST time of enqueueing one call (perf_counter around the call, the
      stream idle before and not waited for after).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def bench(N, opt):
    import torch

    from dir_amd import functional as F
    from dir_amd.engine import run_mano_pair
    from dir_amd.manopth.manolayer import ManoLayer
    from dir_amd.utils import mano_fit as MF
    iters, T = opt.iters, opt.seq
    assert N % T == 0
    S = N // T
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=9, flat_hand_mean=False, side=s).cuda() for s in ('left', 'right')]
    tabs = [m.c_tables(9) for m in layers]
    rng = np.random.default_rng(0)
    truth = []
    for _ in range(2):
        a, b = (rng.normal(0, 1, (S, 1, 64)).astype(np.float32) for _ in range(2))
        t = np.linspace(0, 1, T, dtype=np.float32)[None, :, None]
        z = (a + 0.3 * t * (b - a)).reshape(N, 64)
        p = MF.neutral_para(N, 4.0)
        p[:, :6] += torch.from_numpy(0.2 * z[:, :6]).cuda()
        p[:, 6:51] = torch.from_numpy(0.4 * z[:, 6:51]).cuda()
        p[:, 51:61] = torch.from_numpy(np.repeat(0.4 * a[:, 0, 51:61], T, 0)).cuda()
        truth.append(p)
    (_, jl, _), (_, jr, _) = run_mano_pair(tabs, truth[0], truth[1], N)
    targets = [jl.clone(), jr.clone()]
    cold = [MF.neutral_para(N, 4.0) + 0.02 * torch.randn(N, 64, device='cuda', generator=torch.Generator('cuda').manual_seed(h)) for h in (0, 1)]
    W, LR = {'w_joints': 1e4}, [0.03] * 4
    kj = 2.0 * 1e4 / 21.0
    seq_start = torch.arange(0, N + 1, T, dtype=torch.int32).cuda()
    work = torch.empty(F.mano_fit_sequence_workspace_bytes(N, S, 2), dtype=torch.uint8, device='cuda')

    def seq(share):
        return lambda: F.mano_fit_sequence(tabs, cold, seq_start, joints=targets, iters=iters, lr=LR, weights=W, smooth=(1.0, 1.0, 1.0), share_betas=share, work=work)

    def fit():
        return F.mano_fit(tabs, cold, joints=targets, iters=iters, lr=LR, weights=W)

    def composed():
        ps = [torch.nn.Parameter(c.clone()) for c in cold]
        adam = torch.optim.Adam(ps, lr=0.03, foreach=True)
        for _ in range(iters):
            (_, a, _), (_, b, _) = run_mano_pair(tabs, ps[0].data, ps[1].data, N)
            g = F.mano_backward(tabs, [ps[0].data, ps[1].data], g_joints=[kj * (a - targets[0]), kj * (b - targets[1])])
            ps[0].grad, ps[1].grad = g[0], g[1]
            adam.step()
        return ps
    variants = {'seq_shared': seq(True), 'seq_per_frame': seq(False), 'fit': fit, 'composed': composed}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            fn()
            host[k].append((time.perf_counter() - t0) * 1e6)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0)
    print('N = %d frames x 2 hands in %d sequences of %d, %d iterations, %d rounds, one call per round and variant' % (N, S, T, iters, opt.rounds))
    res = {}
    for k in variants:
        t, h = np.array(times[k]), np.array(host[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max()), 'us_per_iteration': float(np.median(t)) / iters,
                  'host_us_median': float(np.median(h)), 'host_us_per_iteration': float(np.median(h)) / iters}
        print('%-14s %10.1f us  (%.1f .. %.1f)  %8.1f us per iteration   host enqueue %10.1f us = %6.1f us per iteration' % (
            k, res[k]['us_median'], t.min(), t.max(), res[k]['us_per_iteration'], res[k]['host_us_median'], res[k]['host_us_per_iteration']))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, nargs='+', default=[64, 512])
    ap.add_argument('--seq', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=20)
    opt = ap.parse_args()
    print(json.dumps({'bench_mano_seq_fit': {str(N): bench(N, opt) for N in opt.frames}}))


if __name__ == '__main__':
    main()
