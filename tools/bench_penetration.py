"""Measures the inter-hand penetration kernels (csrc/penetration.hip) and what --penetration costs apps.eval, on the GPU.

  python tools/bench_penetration.py kernels [--batch 256] [--rounds 20]
      dir_mesh_penetration and dir_mesh_intersection_volume on MANO-sized pairs from the synthetic table (per-vertex noise 3 mm,
      relative offset 20 mm), HIP events around each call, the two alternating inside one process after a warm-up.  Prints the
      median and the min..max of the rounds beside the point-triangle evaluations computed from the shapes.
  python tools/bench_penetration.py eval --data DIR [--images 16384] [--rounds 3] [--parent TREE]
      images/s of apps.eval.evaluate_from_disk on the fake split (tests/helpers/fake_split.py: 512 files written to DIR when they are not
      there, read round and round until `images` are scored), 256 per batch, synthetic weights: --penetration off, on without volume, on with the 5 mm volume, alternating for `rounds`
      rounds.  --parent TREE: a built checkout of another commit whose unflagged loop joins the alternation in a child process
      per round (its own library cannot share a process with this one).
  python tools/bench_penetration.py eval-child --data DIR --images N      (what --parent runs inside TREE: prints one rate)
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


def kernels(opt):
    import penetration_ref as R
    from dir_amd.utils import penetration as PN
    B = opt.batch
    a, fa, b, fb = R.hand_pairs(B, seed=2)
    A, Bv = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    FA, FB = torch.from_numpy(fa).cuda(), torch.from_numpy(np.ascontiguousarray(fb)).cuda()
    nf = [len(R.valid_faces(f, 778)) for f in (fa, fb)]
    variants = {'penetration': lambda: PN.mesh_penetration(A, FA, Bv, FB),
                'penetration+per_vertex': lambda: PN.mesh_penetration(A, FA, Bv, FB, per_vertex=True),
                'volume_5mm': lambda: PN.intersection_volume(A, FA, Bv, FB)}
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
    vol = PN.intersection_volume(A, FA, Bv, FB)
    cells, n_both = vol['cells'].cpu().numpy().astype(np.int64), vol['n_both'].cpu().numpy().astype(np.int64)
    pen = PN.mesh_penetration(A, FA, Bv, FB)
    evals = {'penetration': B * (a.shape[1] * nf[1] + b.shape[1] * nf[0])}
    evals['penetration+per_vertex'] = evals['penetration']
    evals['volume_5mm'] = None          # cells * F_a + (points inside A) * F_b: the second term is known to the kernel only
    out = {'batch': B, 'verts': [a.shape[1], b.shape[1]], 'valid_faces': nf, 'rounds': opt.rounds, 'inner': opt.inner,
           'lattice_points_total': int(cells.sum()), 'lattice_points_mean': float(cells.mean()), 'inside_both_mean': float(n_both.mean()),
           'volume_evals_lower_bound': int(cells.sum() * nf[0] + n_both.sum() * nf[1]),
           'samples_with_penetration': float((pen['count'].sum(1) > 0).float().mean())}
    for k, t in times.items():
        out[k] = {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t), 'point_triangle_evals': evals[k]}
        if evals[k]:
            out[k]['evals_per_s'] = evals[k] / (statistics.median(t) * 1e-3)
    print(json.dumps(out))


FILES = 512


def _state():
    from dir_amd import synth
    with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def _split(opt):
    from fake_split import write_split
    if not os.path.exists(os.path.join(opt.data, 'test', 'anno', '%d.pkl' % (FILES - 1))):
        write_split(opt.data, FILES, seed=7)


def _loop(eng, mano, jreg, opt, pen):
    from dir_amd.apps import eval as EV
    kw = {} if pen is None else {'penetration': pen}
    _, rate = EV.evaluate_from_disk(eng, opt.data, jreg, mano, bs=256, workers=16, indices=[i % FILES for i in range(opt.images)], **kw)
    assert rate['images'] == opt.images
    print('%s: %.0f images/s' % ('off' if pen is None else 'penetration, volume pitch %s' % pen.volume_pitch, rate['images_per_sec']), file=sys.stderr, flush=True)
    return rate['images_per_sec']


def _setup():
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import eval as EV
    from dir_amd.engine import DirEngine
    state = _state()
    eng = DirEngine(state, dtype=torch.float16, root_joint=0)
    mano = DS.gt_layers_from_checkpoint(state)
    return eng, mano, {s: EV.Jr(mano[s].J_regressor) for s in ('left', 'right')}


def eval_child(opt):
    eng, mano, jreg = _setup()
    _loop(eng, mano, jreg, opt, None)                 # warm-up: page cache, graphs, allocator
    print('RATE %f' % _loop(eng, mano, jreg, opt, None))


def eval_rates(opt):
    from dir_amd.utils import penetration as PN
    from dir_amd.utils.vis_utils import faces_from_layers
    _split(opt)
    eng, mano, jreg = _setup()
    faces = PN.hand_faces(faces_from_layers(mano))[:2]
    make = {'off': lambda: None, 'on': lambda: PN.PenetrationMetrics(faces, volume_pitch=None),
            'on+volume': lambda: PN.PenetrationMetrics(faces, volume_pitch=0.005)}
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
        raise SystemExit('bench_penetration needs the GPU: there is nothing to measure without one')
    if opt.mode == 'kernels':
        opt.rounds = opt.rounds or 20
        kernels(opt)
    else:
        if not opt.data:
            ap.error('--data is needed')
        opt.rounds = opt.rounds or 3
        (eval_rates if opt.mode == 'eval' else eval_child)(opt)
