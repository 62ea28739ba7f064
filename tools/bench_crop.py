"""Measures the crop path of dir_amd.utils.crop / dir_amd.apps.predict on the GPU.  No gates: it prints what it finds.

  python tools/bench_crop.py kernels [--b 64] [--rounds 20] [--reps 20]
      HIP events around --reps back-to-back launches (divided by --reps), one process, warmed, the variants alternating round by round;
      median and range per variant.  The entry points are called directly on outputs allocated once, so that the interval holds kernels
      and not allocations; the host's time to enqueue one call is printed beside it -- where the two are equal the GPU waited for the host
      and the figure is an upper bound of the kernel's time.
      dir_crop_frames at B from 512 x 334 frames (InterHand2.6M's size) and from 1920 x 1080 frames, at s ~ 1 and s ~ 0.25, crops of 256;
      the two matrix kernels at B.  Per variant: microseconds, bytes = the crops written + the source footprint read (the frame rows
      and columns the crop's taps touch, once), and that traffic as a share of the copy ceiling -- a device-to-device copy of 256 MiB
      timed in the same run (read + write bytes over its time).
  python tools/bench_crop.py app --model CKPT [--n 256] [--bs 32] [--workers 8]
      apps.predict on a generated folder of 512 x 334 JPEGs: images/s and how long the GPU loop waited for decoded frames, then the
      same frames already decoded through predict() (crops, forward, records: the GPU's share) and the decode alone.
"""
import argparse
import ctypes
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
    """bytes of the source the crop's taps touch, each once: the rectangle of the frame under the crop (+ the second tap row / column)"""
    s, tx, ty = M[0], M[2], M[5]
    x0, x1 = max(0.0, (0 - tx) / s), min(w - 1.0, (size - 1 - tx) / s + 1)
    y0, y1 = max(0.0, (0 - ty) / s), min(h - 1.0, (size - 1 - ty) / s + 1)
    return int(max(0.0, np.floor(x1) - np.floor(x0) + 1) * max(0.0, np.floor(y1) - np.floor(y0) + 1)) * 3


def kernels(opt):
    import torch

    from dir_amd import _capi
    from dir_amd.utils import crop as CR
    L, P, stream = _capi.lib(), _capi.ptr, _capi.stream_ptr()
    B, size = opt.b, 256
    out = torch.empty(B, size, size, 3, dtype=torch.uint8, device='cuda')
    status = torch.empty(B, dtype=torch.int32, device='cuda')
    Mo, vo = torch.empty(B, 6, dtype=torch.float64, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')

    def frames_call(batch, M, valid):
        buf = batch.cuda()
        args = (P(buf), batch.nbytes, ctypes.c_void_p(buf.data_ptr() + batch._desc_off), P(M), P(valid), B, size, P(out), P(status), stream)
        return lambda: _capi.check(L.dir_crop_frames(*args), 'dir_crop_frames')
    rng = np.random.default_rng(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = {}
    for name, (h, w) in (('512x334', (334, 512)), ('1920x1080', (1080, 1920))):
        batch = CR.FrameBatch([rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)])
        batch.cuda()
        for s in (1.0, 0.25):
            half = size / 2 / s                                                          # the crop's half side in frame pixels
            cx, cy = rng.uniform(w * 0.4, w * 0.6, B), rng.uniform(h * 0.4, h * 0.6, B)
            boxes = np.stack([cx - half * 0.8, cy - half * 0.8, cx + half * 0.8, cy + half * 0.8], 1).astype(np.float32)
            M, valid = CR.crop_matrices_from_boxes(torch.from_numpy(boxes).cuda(), 0.8, size)
            assert bool(valid.all())
            Mh = M.cpu().numpy()
            nbytes = B * size * size * 3 + sum(footprint(h, w, Mh[b], size) for b in range(B))
            want = CR.crop_frames(batch, M, valid, size)
            fn = frames_call(batch, M, valid)
            fn()
            assert torch.equal(out, want) and want.any()                                 # the direct call is the wrapper's call
            variants['crop_frames %s s=%.2f' % (name, s)] = (fn, nbytes)
    boxes = torch.from_numpy(np.float32([[100, 80, 400, 300]] * B)).cuda()
    M0, _ = CR.crop_matrices_from_boxes(boxes, 0.8, size)
    stage = {'pd_mesh_xyz_left': torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 778, 3)).astype(np.float32)).cuda(),
             'pd_mesh_xyz_right': torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 778, 3)).astype(np.float32)).cuda(),
             'pd_proj_left': torch.from_numpy(np.float32([[5, 0.1, 0]] * B)).cuda(), 'pd_proj_right': torch.from_numpy(np.float32([[5, -0.1, 0]] * B)).cuda()}
    box_args = (P(boxes), B, 0.8, size, P(Mo), P(vo), stream)
    mesh_args = (P(stage['pd_mesh_xyz_left']), P(stage['pd_mesh_xyz_right']), P(stage['pd_proj_left']), P(stage['pd_proj_right']), P(M0), B, 0.8, size,
                 P(Mo), P(vo), stream)
    variants['matrices_from_boxes'] = (lambda: _capi.check(L.dir_crop_matrices_from_boxes(*box_args), 'boxes'), B * (16 + 48 + 4))
    variants['matrices_from_meshes'] = (lambda: _capi.check(L.dir_crop_matrices_from_meshes(*mesh_args), 'meshes'), B * (2 * 778 * 12 + 24 + 48 + 48 + 4))
    src = torch.empty(256 << 20, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    variants['copy 256 MiB (the ceiling)'] = (lambda: dst.copy_(src), 2 * src.numel())
    for fn, _ in variants.values():                                                      # warm: allocations, code objects, the H2D copies
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times, hosts = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, (fn, _) in variants.items():
            t, h = timed(fn, e0, e1, opt.reps)
            times[k].append(t)
            hosts[k].append(h)
    ceiling = variants['copy 256 MiB (the ceiling)'][1] / (np.median(times['copy 256 MiB (the ceiling)']) * 1e-6)
    print('B = %d, crops of %d, %d rounds of %d calls; copy ceiling measured here: %.2f TB/s' % (B, size, opt.rounds, opt.reps, ceiling / 1e12))
    res = {}
    for k, (_, nbytes) in variants.items():
        t = np.array(times[k])
        med = float(np.median(t))
        res[k] = {'us_median': med, 'us_min': float(t.min()), 'us_max': float(t.max()), 'host_enqueue_us': float(np.median(hosts[k])), 'bytes': int(nbytes),
                  'share_of_ceiling': nbytes / (med * 1e-6) / ceiling}
        print('%-32s %9.1f us  (%.1f .. %.1f; host enqueue %.1f)  %12d bytes  %5.1f %% of the copy ceiling' % (
            k, med, t.min(), t.max(), res[k]['host_enqueue_us'], nbytes, 100 * res[k]['share_of_ceiling']))
    print(json.dumps({'bench_crop_kernels': res, 'copy_ceiling_TBps': ceiling / 1e12}))


def app(opt):
    import torch
    from PIL import Image

    from dir_amd.engine import DirEngine
    from dir_amd.apps import predict as P
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, 'in'), os.path.join(tmp, 'out')
        os.makedirs(src)
        yy, xx = np.mgrid[0:334, 0:512]
        rng = np.random.default_rng(0)
        boxes = {}
        for i in range(opt.n):
            img = np.stack([127 + 100 * np.sin(xx / (9.0 + i % 7) + c) * np.cos(yy / (13.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (334, 512, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(src, '%d.jpg' % i), quality=92)
            boxes['%d.jpg' % i] = [150, 60, 360, 270]
        with open(os.path.join(tmp, 'boxes.json'), 'w') as f:
            json.dump(boxes, f)
        t0 = time.perf_counter()
        frames = [P.decode_bgr(p) for p in P.list_images([src])]
        dec = time.perf_counter() - t0
        print('host decode alone, one thread: %.1f ms per image' % (1000 * dec / opt.n))
        argv = ['--model', opt.model, '--input', src, '--out', out, '--boxes', os.path.join(tmp, 'boxes.json'), '--bs', str(opt.bs), '--workers', str(opt.workers)]
        P.main(argv)                         # warm: code objects, the engine's tuning
        P.main(argv)
        state = torch.load(opt.model, map_location='cpu', weights_only=False)
        eng = DirEngine(state['net'] if isinstance(state, dict) and 'net' in state else state, dtype=torch.float16, root_joint=0)
        bx = [boxes[os.path.basename(p)] for p in P.list_images([src])]
        P.predict(eng, frames[:opt.bs], bx[:opt.bs], bs=opt.bs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.predict(eng, frames, bx, bs=opt.bs)
        torch.cuda.synchronize()
        gpu = time.perf_counter() - t0
        print('decoded frames through predict() (pack, copy, crops, forward, records): %.2f s, %.0f images/s' % (gpu, opt.n / gpu))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--b', type=int, default=64)
    k.add_argument('--rounds', type=int, default=20)
    k.add_argument('--reps', type=int, default=20)
    a = sub.add_parser('app')
    a.add_argument('--model', required=True)
    a.add_argument('--n', type=int, default=256)
    a.add_argument('--bs', type=int, default=32)
    a.add_argument('--workers', type=int, default=8)
    opt = ap.parse_args()
    {'kernels': kernels, 'app': app}[opt.cmd](opt)


if __name__ == '__main__':
    main()
