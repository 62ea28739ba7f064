"""Measures the One-Euro smoothing (dir_one_euro_step, apps.predict --smooth) on the GPU.  No gates: it prints what it finds.

  python tools/bench_smooth.py kernels [--b 32] [--rounds 10] [--reps 20]
      HIP events around --reps back-to-back calls (divided by --reps), one process, warmed, the variants alternating round by round;
      median and range per variant with the host's time to enqueue one call beside it.  B rows of the PredictionSmoother layout (9
      segments, F = 4887), as
        one_euro   dir_one_euro_step in its steady state (every row updates and counts jitter)
        copy       a device-to-device copy of the bytes the kernel has to move: per row it reads x and five state planes and writes y
                   and five state planes, 12 F floats, half of them read and half written
      The kernel is expected to be launch-bound; the copy of the same bytes says what is left of the time beyond moving them.
  python tools/bench_smooth.py app [--model CKPT] [--sequences 8] [--frames 24] [--rounds 2] [--parent TREE]
      apps.predict --track on a generated folder of sequences (640 x 480 PNGs), without and with --smooth, alternating, after a warm run
      of each: the command's own rate line.  --parent TREE: a built checkout of the parent commit whose unflagged loop joins the
      alternation in a child process (app-child).  Without --model the weights are synthetic (the timing does not depend on them).
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get('DIR_BENCH_TREE')          # app-child: the tree whose dir_amd is measured
sys.path.insert(0, CHILD or ROOT)

import numpy as np  # noqa: E402


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


def kernels(opt):
    import torch

    from dir_amd import _capi
    from dir_amd.utils import smooth as SM
    L, P, stream = _capi.lib(), _capi.ptr, _capi.stream_ptr()
    B = opt.b
    f = SM.OneEuro([(p, d, v) for _, p, d, v in SM.STREAMS], B)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(size=(B, f.F)).astype(np.float32)).cuda()
    y = torch.empty_like(x)
    upd = torch.empty(B, dtype=torch.int32, device='cuda')
    args = (P(x), None, B, f._segs, f.S, f.fps, f.min_cutoff, f.beta, f.d_cutoff, f.max_gap, P(f.state), P(y), P(upd), stream)
    nbytes = 12 * 4 * f.F * B
    pool = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    variants = {'one_euro': lambda: _capi.check(L.dir_one_euro_step(*args), 'dir_one_euro_step'),
                'copy': lambda: pool[nbytes // 2:].copy_(pool[:nbytes // 2])}
    for fn in variants.values():                                                         # warm; after three calls every row counts jitter
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    assert upd.cpu().tolist() == [1] * B
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, hosts = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, fn in variants.items():
            t, h = timed(fn, e0, e1, opt.reps)
            times[k].append(t)
            hosts[k].append(h)
    print('B = %d rows of F = %d floats in %d segments, %d rounds of %d calls, %d bytes moved per call' % (B, f.F, f.S, opt.rounds, opt.reps, nbytes))
    res = {}
    for k in variants:
        t = np.array(times[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max()), 'host_enqueue_us': float(np.median(hosts[k])),
                  'bytes': nbytes}
        print('%-10s %8.1f us  (%.1f .. %.1f; host enqueue %.1f us)' % (k, res[k]['us_median'], t.min(), t.max(), res[k]['host_enqueue_us']))
    print(json.dumps({'bench_smooth_kernels': res}))


def make_video(tmp, sequences, frames):
    from PIL import Image
    src = os.path.join(tmp, 'video')
    yy, xx = np.mgrid[0:480, 0:640]
    rng = np.random.default_rng(0)
    boxes = {}
    for q in range(sequences):
        d = os.path.join(src, 's%02d' % q)
        os.makedirs(d)
        for t in range(frames):
            img = np.stack([127 + 100 * np.sin((xx + 3 * t) / (5.0 + q % 5 + c)) * np.cos(yy / (6.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (480, 640, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(d, '%03d.png' % t))
        boxes['s%02d/000' % q] = [170, 90, 470, 390]
    with open(os.path.join(tmp, 'boxes.json'), 'w') as f:
        json.dump(boxes, f)
    return src


def synthetic_model(tmp):
    import torch

    from dir_amd import synth
    with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    path = os.path.join(tmp, 'synthetic.pth')
    torch.save({'net': {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}}, path)
    return path


def run_predict(argv, out, flags, repeats):
    """the command `repeats` times in this process (the first one warms) -> the rate lines of the later ones"""
    from dir_amd.apps import predict as P
    lines = []
    for k in range(repeats):
        cap = io.StringIO()
        with contextlib.redirect_stdout(cap):
            P.main(argv + ['--out', '%s_%d' % (out, k)] + flags)
        lines.append(cap.getvalue().strip().splitlines()[-1])
    return lines[1:]


def app_child(opt):
    for line in run_predict(json.loads(opt.argv), opt.out, [], 2):
        print('RATE ' + line)


def app(opt):
    with tempfile.TemporaryDirectory() as tmp:
        src = make_video(tmp, opt.sequences, opt.frames)
        model = opt.model or synthetic_model(tmp)
        argv = ['--model', model, '--input', src, '--boxes', os.path.join(tmp, 'boxes.json'), '--track', '--bs', str(opt.sequences)]
        print('%d sequences of %d frames (640 x 480), one forward per frame over all sequences' % (opt.sequences, opt.frames))
        for k in range(opt.rounds):
            for name, flags in (('plain', []), ('--smooth', ['--smooth'])):
                for line in run_predict(argv, os.path.join(tmp, 'out_%s_%d' % (name.strip('-'), k)), flags, 2):
                    print('%-10s %s' % (name, line))
            if opt.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'app-child', '--argv', json.dumps(argv), '--out', os.path.join(tmp, 'out_parent_%d' % k)],
                                   env=dict(os.environ, DIR_BENCH_TREE=os.path.abspath(opt.parent)), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError('the parent tree failed (%d):\n%s' % (r.returncode, r.stderr[-2000:]))
                for line in r.stdout.splitlines():
                    if line.startswith('RATE '):
                        print('%-10s %s' % ('parent', line[5:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--b', type=int, default=32)
    k.add_argument('--rounds', type=int, default=10)
    k.add_argument('--reps', type=int, default=20)
    a = sub.add_parser('app')
    a.add_argument('--model', default=None)
    a.add_argument('--sequences', type=int, default=8)
    a.add_argument('--frames', type=int, default=24)
    a.add_argument('--rounds', type=int, default=2)
    a.add_argument('--parent', type=str, default=None)
    c = sub.add_parser('app-child')
    c.add_argument('--argv', required=True)
    c.add_argument('--out', required=True)
    opt = ap.parse_args()
    {'kernels': kernels, 'app': app, 'app-child': app_child}[opt.cmd](opt)


if __name__ == '__main__':
    main()
