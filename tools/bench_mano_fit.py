"""Measures MANO fitting (dir_mano_fit, utils/mano_fit.py, apps.predict --keypoints) on the GPU.  No gates: it prints what it finds.

  python tools/bench_mano_fit.py kernels [--b 256] [--rounds 20] [--iters 100]
      HIP events, one process, warmed, the variants alternating round by round; median and range per variant.  B x 2 hands, mesh targets
      generated from random parameters, cold start, as
        fit_1 / fit_N     dir_mano_fit with iters = 1 and iters = N: one launch each
        composed_N        the same N iterations as a user of the launches that existed before would write them: dir_mano_forward_pair, ATen
                          residual operations, F.mano_backward (dir_mano_backward_pair) and a foreach torch.optim.Adam, per iteration
        fwd_bwd           one dir_mano_forward_pair + one dir_mano_backward_pair: the floor of an iteration built from the two kernels
      Reported: microseconds per call, microseconds per iteration and the ratios.
  python tools/bench_mano_fit.py app [--model CKPT] [--images 64] [--rounds 2] [--parent TREE]
      apps.predict on a generated folder of 640 x 480 PNGs without and with --keypoints (the keypoints: a first run's own 2-D joints shifted
      by a few pixels), alternating, after a warm run of each: the command's own rate line.  --parent TREE: a built checkout of the parent
      commit whose unflagged loop joins the alternation in a child process (app-child).  Without --model the weights are synthetic.
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get('DIR_BENCH_TREE')          # app-child: the tree whose dir_amd is measured
sys.path.insert(0, CHILD or ROOT)

import numpy as np  # noqa: E402


def kernels(opt):
    import torch

    from dir_amd import functional as F
    from dir_amd.engine import run_mano_pair
    from dir_amd.manopth.manolayer import ManoLayer
    from dir_amd.utils import mano_fit as MF
    B, N = opt.b, opt.iters
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=9, flat_hand_mean=False, side=s).cuda() for s in ('left', 'right')]
    tabs = [m.c_tables(9) for m in layers]
    rng = np.random.default_rng(0)
    truth = []
    for _ in range(2):
        p = MF.neutral_para(B, 4.0)
        p[:, :6] += torch.from_numpy(rng.normal(0, 0.2, (B, 6)).astype(np.float32)).cuda()
        p[:, 6:61] = torch.from_numpy(rng.normal(0, 0.4, (B, 55)).astype(np.float32)).cuda()
        truth.append(p)
    (tl, _, _), (tr, _, _) = run_mano_pair(tabs, truth[0], truth[1], B)
    targets = [tl.clone(), tr.clone()]
    cold = [MF.neutral_para(B, 4.0), MF.neutral_para(B, 4.0)]
    W, LR = {'w_verts': 1e4}, [0.03] * 4
    kv = 2.0 * 1e4 / 778.0

    def fit(n):
        return lambda: F.mano_fit(tabs, cold, verts=targets, iters=n, lr=LR, weights=W)

    def composed():
        ps = [torch.nn.Parameter(c.clone()) for c in cold]
        adam = torch.optim.Adam(ps, lr=0.03, foreach=True)
        for _ in range(N):
            (vl, _, _), (vr, _, _) = run_mano_pair(tabs, ps[0].data, ps[1].data, B)
            g = F.mano_backward(tabs, [ps[0].data, ps[1].data], g_verts=[kv * (vl - targets[0]), kv * (vr - targets[1])])
            ps[0].grad, ps[1].grad = g[0], g[1]
            adam.step()
        return ps

    def fwd_bwd():
        (vl, _, _), (vr, _, _) = run_mano_pair(tabs, cold[0], cold[1], B)
        F.mano_backward(tabs, cold, g_verts=[vl, vr])
    variants = {'fit_1': (fit(1), 1), 'fit_%d' % N: (fit(N), N), 'composed_%d' % N: (composed, N), 'fwd_bwd': (fwd_bwd, 1)}
    for fn, _ in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, b = fit(N)(), composed()
    torch.cuda.synchronize()
    print('after %d iterations: worst vertex RMS %.3f mm (dir_mano_fit), largest parameter difference to the composed loop %.3g' % (
        N, float(torch.stack([r['mse'][:, 3] for r in a]).sqrt().max()) * 1e3, max(float((r['para'] - p.data).abs().max()) for r, p in zip(a, b))))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, (fn, _) in variants.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0)
    print('B = %d x 2 hands, %d rounds, one call per round and variant' % (B, opt.rounds))
    res = {}
    for k, (_, n) in variants.items():
        t = np.array(times[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max()), 'us_per_iteration': float(np.median(t)) / n}
        print('%-14s %10.1f us  (%.1f .. %.1f)  %8.1f us per iteration' % (k, res[k]['us_median'], t.min(), t.max(), res[k]['us_per_iteration']))
    fN, cN = res['fit_%d' % N]['us_per_iteration'], res['composed_%d' % N]['us_per_iteration']
    print('per iteration: composed / fit = %.2f, fit / (forward + backward) = %.2f' % (cN / fN, fN / res['fwd_bwd']['us_median']))
    print(json.dumps({'bench_mano_fit_kernels': res}))


def make_images(tmp, n):
    from PIL import Image
    src = os.path.join(tmp, 'images')
    os.makedirs(src)
    yy, xx = np.mgrid[0:480, 0:640]
    rng = np.random.default_rng(0)
    for t in range(n):
        img = np.stack([127 + 100 * np.sin((xx + 3 * t) / (5.0 + t % 5 + c)) * np.cos(yy / (6.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (480, 640, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(src, '%03d.png' % t))
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
        src = make_images(tmp, opt.images)
        model = opt.model or synthetic_model(tmp)
        argv = ['--model', model, '--input', src, '--bs', '32']
        run_predict(argv, os.path.join(tmp, 'first'), [], 1)
        kps = {}
        for n in sorted(os.listdir(os.path.join(tmp, 'first_0'))):
            with open(os.path.join(tmp, 'first_0', n)) as f:
                r = json.load(f)
            kps[r['image']] = {s: [[x + 3.0, y - 2.0, 1.0] for x, y in r[s]['joints_px']] for s in ('left', 'right')}
        with open(os.path.join(tmp, 'kp.json'), 'w') as f:
            json.dump(kps, f)
        print('%d images (640 x 480), batches of 32' % opt.images)
        for k in range(opt.rounds):
            for name, flags in (('plain', []), ('--keypoints', ['--keypoints', os.path.join(tmp, 'kp.json')])):
                for line in run_predict(argv, os.path.join(tmp, 'out_%s_%d' % (name.strip('-'), k)), flags, 2):
                    print('%-12s %s' % (name, line))
            if opt.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'app-child', '--argv', json.dumps(argv), '--out', os.path.join(tmp, 'out_parent_%d' % k)],
                                   env=dict(os.environ, DIR_BENCH_TREE=os.path.abspath(opt.parent)), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError('the parent tree failed (%d):\n%s' % (r.returncode, r.stderr[-2000:]))
                for line in r.stdout.splitlines():
                    if line.startswith('RATE '):
                        print('%-12s %s' % ('parent', line[5:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--b', type=int, default=256)
    k.add_argument('--rounds', type=int, default=20)
    k.add_argument('--iters', type=int, default=100)
    a = sub.add_parser('app')
    a.add_argument('--model', default=None)
    a.add_argument('--images', type=int, default=64)
    a.add_argument('--rounds', type=int, default=2)
    a.add_argument('--parent', type=str, default=None)
    c = sub.add_parser('app-child')
    c.add_argument('--argv', required=True)
    c.add_argument('--out', required=True)
    opt = ap.parse_args()
    {'kernels': kernels, 'app': app, 'app-child': app_child}[opt.cmd](opt)


if __name__ == '__main__':
    main()
