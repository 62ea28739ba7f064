"""Measures the anti-aliased crop (dir_crop_frames_area) on the GPU.  No gates: it prints what it finds.

  python tools/bench_crop_area.py kernels [--b 64] [--rounds 10] [--reps 10]
      HIP events around --reps back-to-back calls (divided by --reps), one process, warmed, the variants alternating round by round; outputs
      allocated once; median and range per variant, the host's time to enqueue one call beside it.  B crops of 256 from 1920 x 1080 and
      3840 x 2160 frames at s ~ 0.5, 0.25 and 0.12, each as
        area    dir_crop_frames_area
        plain   dir_crop_frames on the same inputs: the four-tap crop, which reads far fewer bytes -- a ratio to report, not a gate (its
                line shows `area`'s byte count, so the TB/s printed for it is not a rate it reaches)
        copy    a device-to-device copy that moves as many bytes as `area` has to (the crops written + the source footprint read: the
                frame rows and columns under the crop's windows, each once), half of them read and half written: the bandwidth yardstick
      and per (frame, s) the ratio area / plain and the share of the copy's rate that `area` reaches.
  python tools/bench_crop_area.py app [--model CKPT] [--n 64] [--bs 32] [--workers 8]
      apps.predict on a generated folder of 1920 x 1080 JPEGs with 900 px hand boxes (s = 0.23), without and with --antialias, alternating,
      twice each after a warm run: the command's own last two lines (images/s and the wait for decoded frames).  Without --model the
      weights are synthetic (the timing does not depend on them).
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, e0, e1, reps):
    """-> (microseconds per call between the events, microseconds the host took to enqueue one call)"""
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps, host * 1e6 / reps


def footprint(h, w, M, size):
    """bytes of the frame under the anti-aliased crop's windows, each once (include/dir_hip.h: first tap of position 0 .. last tap of
    position size - 1 per axis, clipped to the frame)"""
    n = []
    for s, t, lim in ((M[0], M[2], w), (M[4], M[5], h)):
        in0 = 0.5 - (t + 0.5) / s
        scale = (in0 + size / s - in0) / size
        fs = max(scale, 1.0)
        lo = np.floor(in0 + 0.5 * scale - fs + 0.5)
        hi = np.floor(in0 + (size - 0.5) * scale + fs + 0.5)
        n.append(max(0.0, min(hi, lim) - max(lo, 0.0)))
    return int(n[0] * n[1]) * 3


def kernels(opt):
    import torch

    from dir_amd import _capi
    from dir_amd.utils import crop as CR
    L, P, stream = _capi.lib(), _capi.ptr, _capi.stream_ptr()
    B, size = opt.b, 256
    out = torch.empty(B, size, size, 3, dtype=torch.uint8, device='cuda')
    status = torch.empty(B, dtype=torch.int32, device='cuda')
    area = torch.empty(B, dtype=torch.int32, device='cuda')
    pool = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')                        # the copy's source and destination: 512 MiB each
    rng = np.random.default_rng(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants, groups = {}, []
    for name, (h, w) in (('1920x1080', (1080, 1920)), ('3840x2160', (2160, 3840))):
        frame = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        batch = CR.FrameBatch([frame] * B)                                               # B copies at B places: the kernel does not look at the values
        buf = batch.cuda()
        descs = ctypes.c_void_p(buf.data_ptr() + batch._desc_off)
        for s in (0.5, 0.25, 0.12):
            half = size / 2 / s                                                          # the crop's half side in frame pixels
            cx, cy = rng.uniform(w * 0.4, w * 0.6, B), rng.uniform(h * 0.4, h * 0.6, B)
            boxes = np.stack([cx - half * 0.8, cy - half * 0.8, cx + half * 0.8, cy + half * 0.8], 1).astype(np.float32)
            M, valid = CR.crop_matrices_from_boxes(torch.from_numpy(boxes).cuda(), 0.8, size)
            assert bool(valid.all())
            Mh = M.cpu().numpy()
            nbytes = B * size * size * 3 + sum(footprint(h, w, Mh[b], size) for b in range(B))
            a_args = (P(buf), batch.nbytes, descs, P(M), P(valid), B, size, P(out), P(status), P(area), stream)
            p_args = a_args[:9] + (stream,)
            want, flags = CR.crop_frames(batch, M, valid, size, antialias=True, return_area=True)
            _capi.check(L.dir_crop_frames_area(*a_args), 'dir_crop_frames_area')
            assert torch.equal(out, want) and want.any() and bool(flags.all()) and bool((status == 0).all())      # the direct call is the wrapper's
            half_n = min(nbytes // 2, pool.numel() // 2)
            key = '%s s=%.2f' % (name, s)
            variants[key + ' area'] = (lambda a=a_args: _capi.check(L.dir_crop_frames_area(*a), 'dir_crop_frames_area'), nbytes)
            variants[key + ' plain'] = (lambda a=p_args: _capi.check(L.dir_crop_frames(*a), 'dir_crop_frames'), nbytes)
            variants[key + ' copy'] = (lambda n=half_n: pool[pool.numel() // 2:pool.numel() // 2 + n].copy_(pool[:n]), 2 * half_n)
            groups.append(key)
    for fn, _ in variants.values():                                                      # warm: code objects, the H2D copies
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times, hosts = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, (fn, _) in variants.items():
            t, hst = timed(fn, e0, e1, opt.reps)
            times[k].append(t)
            hosts[k].append(hst)
    print('B = %d, crops of %d, %d rounds of %d calls' % (B, size, opt.rounds, opt.reps))
    res = {}
    for k, (_, nbytes) in variants.items():
        t = np.array(times[k])
        med = float(np.median(t))
        res[k] = {'us_median': med, 'us_min': float(t.min()), 'us_max': float(t.max()), 'host_enqueue_us': float(np.median(hosts[k])), 'bytes': int(nbytes),
                  'TBps': nbytes / (med * 1e-6) / 1e12}
        print('%-28s %9.1f us  (%.1f .. %.1f; host enqueue %.1f)  %12d bytes  %5.2f TB/s' % (
            k, med, t.min(), t.max(), res[k]['host_enqueue_us'], nbytes, res[k]['TBps']))
    for key in groups:
        a, p, c = (res[key + ' ' + v] for v in ('area', 'plain', 'copy'))
        res[key] = {'area_over_plain': a['us_median'] / p['us_median'], 'share_of_copy_rate': a['TBps'] / c['TBps']}
        print('%-22s area / plain = %5.1f x   area reaches %5.1f %% of the copy rate for its bytes' % (
            key, res[key]['area_over_plain'], 100 * res[key]['share_of_copy_rate']))
    print(json.dumps({'bench_crop_area_kernels': res}))


def app(opt):
    import torch
    from PIL import Image

    from dir_amd import synth
    from dir_amd.apps import predict as P
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, 'in')
        os.makedirs(src)
        model = opt.model
        if model is None:
            with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as fh:
                shapes = {k: tuple(v) for k, v in json.load(fh).items()}
            model = os.path.join(tmp, 'synthetic.pth')
            torch.save({'net': {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}}, model)
        yy, xx = np.mgrid[0:1080, 0:1920]
        rng = np.random.default_rng(0)
        boxes = {}
        for i in range(opt.n):
            img = np.stack([127 + 100 * np.sin(xx / (3.0 + i % 7) + c) * np.cos(yy / (4.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (1080, 1920, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(src, '%d.jpg' % i), quality=92)
            boxes['%d.jpg' % i] = [500, 90, 1400, 990]
        with open(os.path.join(tmp, 'boxes.json'), 'w') as f:
            json.dump(boxes, f)
        argv = ['--model', model, '--input', src, '--boxes', os.path.join(tmp, 'boxes.json'), '--bs', str(opt.bs), '--workers', str(opt.workers)]

        def once(flag, k):
            cap = io.StringIO()
            with contextlib.redirect_stdout(cap):
                P.main(argv + ['--out', os.path.join(tmp, 'out%d%d' % (len(flag), k))] + flag)
            return ' | '.join(cap.getvalue().strip().splitlines()[-2:])
        once([], 0)                              # warm: code objects, the engine's tuning
        once(['--antialias'], 0)
        for k in (1, 2):
            for flag in ([], ['--antialias']):
                print('%-12s %s' % (' '.join(flag) or 'plain', once(flag, k)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--b', type=int, default=64)
    k.add_argument('--rounds', type=int, default=10)
    k.add_argument('--reps', type=int, default=10)
    a = sub.add_parser('app')
    a.add_argument('--model', default=None)
    a.add_argument('--n', type=int, default=64)
    a.add_argument('--bs', type=int, default=32)
    a.add_argument('--workers', type=int, default=8)
    opt = ap.parse_args()
    {'kernels': kernels, 'app': app}[opt.cmd](opt)


if __name__ == '__main__':
    main()
