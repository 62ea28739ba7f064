"""The guarded AdamW step at the model's size (92.7 M fp32 parameters), HIP events in one process, warmed, the variants alternating:

  plain        dir_adamw_step                                   4 reads + 3 writes x 4 B per element          2.60 GB
  guarded      dir_grad_guard + dir_adamw_guarded_step          + 1 read of the gradient for the norm         2.97 GB
  guarded+ema  ... with the average                             + 1 read + 1 write of the average             3.71 GB
  copy B       a device copy that moves the same bytes (B / 2 read, B / 2 written): what the memory system gives for that traffic

    python tools/bench_guarded_step.py [--n 92730000] [--rounds 30] [--train-step] [--parent DIR]

--train-step: also the graph-captured 32-image training step (GraphedTrainStep) with the three features off, in a child process of its own;
--parent DIR: ... and the same in a built checkout of the parent commit at DIR (another child process).  No gate: the step is expected to be
unchanged, because with the flags off FlatAdamW.step() is the code it was."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(n, rounds):
    import ctypes
    import torch
    sys.path.insert(0, ROOT)
    from dir_amd import _capi
    L = _capi.lib()
    p, g = (torch.randn(n, device='cuda') * 0.01 for _ in range(2))
    m, v = (torch.zeros(n, device='cuda') for _ in range(2))
    e = p.clone()
    state = torch.zeros(ctypes.sizeof(_capi.GuardState), dtype=torch.uint8, device='cuda')
    ws = torch.zeros(L.dir_grad_norm_workspace_bytes(n) // 8, dtype=torch.float64, device='cuda')
    src = torch.empty(n * 5, device='cuda')              # 5 n floats: the largest copy below reads 3.71 GB / 2
    dst = torch.empty(n * 5, device='cuda')
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    count = [0]

    def plain():
        count[0] += 1
        _capi.check(L.dir_adamw_step(_capi.ptr(p), _capi.ptr(g), _capi.ptr(m), _capi.ptr(v), n, *hyper, count[0], _capi.stream_ptr()), 'plain')

    def guarded(ema):
        s = _capi.stream_ptr()
        _capi.check(L.dir_grad_guard(_capi.ptr(g), n, 1.0, 1, 0.9, 0.999, _capi.ptr(ws), ws.numel() * 8, _capi.ptr(state), s), 'guard')
        _capi.check(L.dir_adamw_guarded_step(_capi.ptr(p), _capi.ptr(g), _capi.ptr(m), _capi.ptr(v), _capi.ptr(e) if ema else None, n, *hyper,
                                             0.9998 if ema else 0.0, _capi.ptr(state), s), 'guarded')

    def copy(nbytes):
        k = nbytes // 8                                      # floats read = floats written
        return lambda: dst[:k].copy_(src[:k])
    traffic = {'plain': 28 * n, 'guarded': 32 * n, 'guarded+ema': 40 * n}
    variants = [('plain', plain), ('guarded', lambda: guarded(False)), ('guarded+ema', lambda: guarded(True))]
    variants += [('copy %s' % k, copy(b)) for k, b in traffic.items()]
    times = {k: [] for k, _ in variants}
    for r in range(rounds + 3):
        for k, fn in variants:                               # alternating: every variant sees the same clocks and neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:                                       # three warm rounds
                times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {}
    for k, _ in variants:
        b = traffic[k.replace('copy ', '')]
        us = statistics.median(times[k])
        res[k] = {'us': us, 'min_us': min(times[k]), 'GB': b / 1e9, 'GB_per_s': b / us / 1e3}
        print('%-18s %8.1f us median (%8.1f min)  %.2f GB  %6.0f GB/s' % (k, us, min(times[k]), b / 1e9, b / us / 1e3))
    return res


TRAIN_CHILD = r'''
import json, os, sys, time
import numpy as np, torch
ROOT = sys.argv[1]; B = int(sys.argv[2]); sys.path.insert(0, ROOT)
from dir_amd import synth
from dir_amd.optim import FlatAdamW
from dir_amd.train import step as TSTEP
shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json'))).items()}
sd = synth.synth_state_dict(shapes, 1234)
is_buf = lambda k: any(t in k for t in ('running_', 'num_batches', 'mano_layer', 'img_gird', 'seg_loss.weight'))
params = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in sd.items() if not is_buf(k)}
buffers = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items() if is_buf(k) and 'num_batches' not in k}
opt = FlatAdamW(list(params.values()), lr=1e-5); opt.set_inactive(TSTEP.inactive_parameters(params))
rng = np.random.RandomState(0)
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
img = dv(synth.synth_input('train.img.0', (B, 3, 256, 256), 1234))
target, meta = {}, {}
for s in ('left', 'right'):
    target['joint_2d_' + s] = dv(rng.uniform(-1, 1, (B, 21, 3)).astype(np.float32)); target['mesh_2d_' + s] = dv(rng.uniform(-1, 1, (B, 778, 3)).astype(np.float32))
    target['joint_3d_' + s] = dv(rng.normal(0, 0.05, (B, 21, 3)).astype(np.float32)); target['mesh_3d_' + s] = dv(rng.normal(0, 0.05, (B, 778, 3)).astype(np.float32))
    meta['center_' + s] = dv(rng.normal(0, 0.1, (B, 1, 3)).astype(np.float32))
target['seg'] = dv(rng.randint(0, 3, (B, 1, 256, 256)).astype(np.float32)); target['dense'] = dv(rng.rand(B, 3, 256, 256).astype(np.float32))
faces = tuple(dv(synth.loss_faces(s, 1234).astype(np.int64)) for s in ('left', 'right'))
gs = TSTEP.GraphedTrainStep(params, buffers, opt, faces)
for i in range(8):
    gs(img, target, meta)
torch.cuda.synchronize()
ts = []
for r in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(5):
        gs(img, target, meta)
    e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / 5)
print('TRAIN_STEP_MS ' + json.dumps({'median': sorted(ts)[2], 'min': min(ts), 'all': ts}))
'''


def train_step(root, batch):
    """the graphed training step of the tree at `root`, flags off, in a fresh child process -> {'median', 'min', 'all'} (ms) or None"""
    r = subprocess.run([sys.executable, '-c', TRAIN_CHILD, root, str(batch)], capture_output=True, text=True, cwd=root)
    for line in r.stdout.split('\n'):
        if line.startswith('TRAIN_STEP_MS '):
            return json.loads(line[len('TRAIN_STEP_MS '):])
    print('the training step in %s did not finish (exit %d):\n%s' % (root, r.returncode, r.stderr[-2000:]))
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=92_730_000)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--train-step', action='store_true')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--parent', type=str, default=None, help='a built checkout of the parent commit')
    ap.add_argument('--json', type=str, default=None, help='write every figure here')
    opt = ap.parse_args(argv)
    res = {'n': opt.n, 'kernels': kernels(opt.n, opt.rounds)}
    if opt.train_step:
        for name, root in (('this', ROOT), ('parent', opt.parent)):
            if root is None:
                print('graphed training step, %s: not measured (no --parent)' % name)
                continue
            t = train_step(os.path.abspath(root), opt.batch)
            res['train_step_' + name] = t
            if t is not None:
                print('graphed training step, %d images, flags off, %-6s: %.2f ms median of 5 x 5 (%.2f min)' % (opt.batch, name, t['median'], t['min']))
    if opt.json:
        with open(opt.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    assert all(math.isfinite(v['us']) for v in res['kernels'].values())
    return res


if __name__ == '__main__':
    main()
