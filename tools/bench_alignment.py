"""Measures the aligned-evaluation kernels (csrc/alignmetric.hip) and what --aligned costs apps.eval, on the GPU.

  python tools/bench_alignment.py kernels [--batch 256] [--rounds 20]
      dir_procrustes_align, dir_point_set_nn and dir_threshold_counts at N = 21 and N = 778 on the seeded pairs of
      tests/helpers/alignment_ref.py, and one AlignedMetrics.update per batch; HIP events around each window of calls, the variants
      alternating inside one process after a warm-up.  Prints the median and the min..max of the rounds.
  python tools/bench_alignment.py eval --data DIR [--images 16384] [--rounds 3] [--parent TREE]
      images/s of apps.eval.evaluate_from_disk on the fake split (tests/helpers/fake_split.py: 512 files written to DIR when they are not
      there, read round and round until `images` are scored), 256 per batch, synthetic weights: --aligned off and on, alternating for
      `rounds` rounds.  --parent TREE: a built checkout of another commit whose unflagged loop joins the alternation in a child process
      per round (its own library cannot share a process with this one).
  python tools/bench_alignment.py eval-child --data DIR --images N      (what --parent runs inside TREE: prints one rate)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get('DIR_BENCH_TREE')          # eval-child: the tree whose dir_amd is measured
sys.path.insert(0, CHILD or ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests', 'helpers'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _state():
    from dir_amd import synth
    with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def _setup(engine=True):
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import eval as EV
    from dir_amd.engine import DirEngine
    state = _state()
    eng = DirEngine(state, dtype=torch.float16, root_joint=0) if engine else None
    mano = DS.gt_layers_from_checkpoint(state)
    return eng, mano, {s: EV.Jr(mano[s].J_regressor) for s in ('left', 'right')}


def kernels(opt):
    import alignment_ref as R
    from dir_amd.utils import alignment as AL
    B = opt.batch
    pd, gt = R.pairs(B, seed=2)
    sub = list(R.SUBSET21)
    P, G = torch.from_numpy(pd).cuda(), torch.from_numpy(gt).cuda()
    P21, G21 = P[:, sub].contiguous(), G[:, sub].contiguous()
    A = AL.procrustes_align(P, G, want_aligned=True)
    A21 = AL.procrustes_align(P21, G21, want_aligned=True)
    thr = torch.from_numpy(AL.default_thresholds().astype(np.float32)).cuda()
    counts = torch.zeros(101, dtype=torch.int64, device='cuda')
    _, _, jreg = _setup(engine=False)
    g = np.random.default_rng(3)
    pr, gr = R.pairs(B, seed=4)
    result = [None, None, {'pd_mesh_xyz_left': P, 'pd_mesh_xyz_right': torch.from_numpy(pr).cuda(),
                           'pd_offset': torch.from_numpy(g.normal(0, 0.3, (B, 3)).astype(np.float32)).cuda()}]
    cam = torch.from_numpy(np.tile(np.array([[1500.0, 0, 128], [0, 1500.0, 128], [0, 0, 1]], np.float32), (B, 1, 1))).cuda()
    v2d = torch.from_numpy(g.uniform(0, 256, (B, 778, 2)).astype(np.float32)).cuda()
    data = (None, None, None, G, None, torch.from_numpy(gr).cuda(), None, v2d, None, v2d, cam)
    metrics = AL.AlignedMetrics(jreg)

    def update():
        metrics.update(result, data)
        metrics.batches.clear()                     # the per-sample results of a timing loop are not kept

    variants = {'procrustes_21': lambda: AL.procrustes_align(P21, G21, want_aligned=True),
                'procrustes_778': lambda: AL.procrustes_align(P, G, want_aligned=True),
                'nn_21': lambda: AL.nn_distances(A21['aligned'], G21),
                'nn_778': lambda: AL.nn_distances(A['aligned'], G),
                'counts_21': lambda: AL.threshold_counts(A21['err'], thr, counts),
                'counts_778': lambda: AL.threshold_counts(A['err'], thr, counts),
                'aligned_metrics_update': update}
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(opt.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / opt.inner)
    out = {'batch': B, 'rounds': opt.rounds, 'inner': opt.inner, 'nn_778_distance_evaluations': 2 * B * 778 * 778,
           'procrustes_778_bytes': B * 778 * (12 * 2 * 3 + 12 + 4)}
    for k, t in times.items():
        out[k] = {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t)}
    out['nn_778']['evals_per_s'] = out['nn_778_distance_evaluations'] / (out['nn_778']['median_ms'] * 1e-3)
    print(json.dumps(out))


FILES = 512


def _split(opt):
    from fake_split import write_split
    if not os.path.exists(os.path.join(opt.data, 'test', 'anno', '%d.pkl' % (FILES - 1))):
        write_split(opt.data, FILES, seed=7)


def _loop(eng, mano, jreg, opt, aligned):
    from dir_amd.apps import eval as EV
    kw = {} if aligned is None else {'aligned': aligned}
    _, rate = EV.evaluate_from_disk(eng, opt.data, jreg, mano, bs=256, workers=16, indices=[i % FILES for i in range(opt.images)], **kw)
    assert rate['images'] == opt.images
    print('%s: %.0f images/s' % ('off' if aligned is None else 'aligned', rate['images_per_sec']), file=sys.stderr, flush=True)
    return rate['images_per_sec']


def eval_child(opt):
    eng, mano, jreg = _setup()
    _loop(eng, mano, jreg, opt, None)                 # warm-up: page cache, graphs, allocator
    print('RATE %f' % _loop(eng, mano, jreg, opt, None))


def eval_rates(opt):
    from dir_amd.utils.alignment import AlignedMetrics
    _split(opt)
    eng, mano, jreg = _setup()
    make = {'off': lambda: None, 'aligned': lambda: AlignedMetrics(jreg)}
    for k in make:
        _loop(eng, mano, jreg, opt, make[k]())
    rates = {k: [] for k in make}
    if opt.parent:
        rates['parent_off'] = []
    for _ in range(opt.rounds):
        for k in make:
            rates[k].append(_loop(eng, mano, jreg, opt, make[k]()))
        if opt.parent:
            t0 = time.time()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), 'eval-child', '--data', opt.data, '--images', str(opt.images)],
                               env=dict(os.environ, DIR_BENCH_TREE=os.path.abspath(opt.parent)), capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError('the parent tree failed (%d) after %.0f s:\n%s' % (r.returncode, time.time() - t0, r.stderr[-2000:]))
            rates['parent_off'].append(float([l for l in r.stdout.splitlines() if l.startswith('RATE ')][-1].split()[1]))
    out = {'images': opt.images, 'batch': 256, 'rounds': opt.rounds}
    for k, r in rates.items():
        out[k] = {'median_images_per_s': statistics.median(r), 'min': min(r), 'max': max(r), 'all': r}
    print(json.dumps(out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'eval', 'eval-child'])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--inner', type=int, default=50, help='calls per timed window')
    ap.add_argument('--data', type=str, default=None)
    ap.add_argument('--images', type=int, default=16384)
    ap.add_argument('--parent', type=str, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_alignment needs the GPU: there is nothing to measure without one')
    if opt.mode == 'kernels':
        opt.rounds = opt.rounds or 20
        kernels(opt)
    else:
        if not opt.data:
            ap.error('--data is needed')
        opt.rounds = opt.rounds or 3
        (eval_rates if opt.mode == 'eval' else eval_child)(opt)
