"""Writes tests/golden/g24_val_metrics.npz: the per-batch validation metric of the reference's training loop, computed by the REFERENCE's
own InterHandDataset.evaluate (dataset/interhand.py:262-315) on the CPU.  Authoring only: it imports the reference tree (path:
$DIR_REFERENCE, default ../reference next to the repository), which never travels with the tests.  cv2, imgaug, yacs and torchvision are
stubbed: evaluate() calls none of them (nor `self`: it is called unbound, with None).

  python tools/gen_val_metric_golden.py

The inputs are regenerated from a seed (tests/helpers/val_metric_ref.py::make_case), so the file stays small.  Per case c:
  seed.c, B.c, n_stages.c, exact.c    the arguments of make_case
  checksum.c                          float64 sum of every input array (a generator that drifted is noticed)
  ref32.c  [n_stages,4] float32       evaluate() on the float32 inputs, per stage: joint left, joint right, vert left, vert right (mm)
  ref64.c  [n_stages,4] float64       evaluate() on float64 copies of the same inputs
  in.0.*                              the input arrays of case 0 themselves (B = 1)"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('DIR_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
OUT = os.path.join(REPO, 'tests', 'golden', 'g24_val_metrics.npz')
sys.path.insert(0, os.path.join(REPO, 'tests', 'helpers'))

# (seed, B, n_stages, exact): B = 1, 4, 5, 32, 64 with 3 and 5 stages; three B = 5 batches of 3 stages (the accumulation test); two
# cases whose predictions equal the ground truth (exactly 0)
CASES = [(2400, 1, 3, False), (2401, 5, 3, False), (2402, 64, 3, False), (2403, 1, 5, False), (2404, 5, 5, False), (2405, 64, 5, False),
         (2406, 4, 3, False), (2407, 32, 3, False), (2408, 5, 3, False), (2409, 5, 3, False), (2410, 5, 3, True), (2411, 64, 5, True)]


def import_ref_dataset():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod('cv2')
    mod('imgaug')
    sys.modules['imgaug'].augmenters = mod('imgaug.augmenters')
    mod('yacs')

    class CfgNode(dict):
        def __init__(self, *a, **k):
            super().__init__()
    mod('yacs.config', CfgNode=CfgNode)
    mod('torchvision')
    sys.modules['torchvision'].transforms = mod('torchvision.transforms')
    import dataset.interhand as D
    return D


def main():
    import torch
    import val_metric_ref as R
    D = import_ref_dataset()
    evaluate = D.InterHandDataset.evaluate
    g = {'cases': np.int64(len(CASES))}
    for c, (seed, B, n_stages, exact) in enumerate(CASES):
        outs_list, targets = R.make_case(seed, B, n_stages, exact)
        g['seed.%d' % c], g['B.%d' % c], g['n_stages.%d' % c], g['exact.%d' % c] = np.int64(seed), np.int64(B), np.int64(n_stages), np.bool_(exact)
        g['checksum.%d' % c] = np.float64(R.checksum(outs_list, targets))
        for name, dt, tdt in (('ref32', np.float32, torch.float32), ('ref64', np.float64, torch.float64)):
            t = {k: torch.from_numpy(v).to(tdt) for k, v in targets.items()}
            rows = []
            for o in outs_list:
                r = evaluate(None, {k: torch.from_numpy(v).to(tdt) for k, v in o.items()}, t, None)
                assert all(np.asarray(x).dtype == dt for x in r), [np.asarray(x).dtype for x in r]
                rows.append(np.array(r, dt))
            g['%s.%d' % (name, c)] = np.stack(rows)
        if c == 0:
            for k, v in targets.items():
                g['in.0.gt.' + k] = v
            for s, o in enumerate(outs_list):
                for k, v in o.items():
                    g['in.0.s%d.%s' % (s, k)] = v
        print('case %2d  B %2d  stages %d  exact %d  ref32 %s  |ref32-ref64| max %.3g' % (
            c, B, n_stages, exact, g['ref32.%d' % c][-1], np.max(np.abs(g['ref32.%d' % c].astype(np.float64) - g['ref64.%d' % c]))))
    np.savez_compressed(OUT, **g)
    print('wrote %s (%d cases, %d arrays, %d bytes)' % (OUT, len(CASES), len(g), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
