"""Writes tests/golden/g25_crop.npz: what the REFERENCE's own cut_img (dataset/dataset_utils.py:26-58) hands to OpenCV and returns, on the
CPU.  Authoring only: it imports the reference tree (path: $DIR_REFERENCE, default ../reference next to the repository), which never
travels with the tests.  cv2 is stubbed with a warpAffine that returns a copy of the matrix it was handed, so the "image" cut_img
returns is that matrix.

  python tools/gen_crop_golden.py

The inputs are regenerated from a seed (tests/helpers/crop_ref.py::make_case: float64 labels, so that cut_img computes in float64), so
the file stays small.  One array per field, the cases stacked along the first axis (C cases):
  seed, ratio, size  [C]      the arguments
  checksum  [C]               float64 sum of every input array (a generator that drifted is noticed)
  matrix    [C,2,3] float64   the matrix cut_img passed to cv.warpAffine
  labels    [C,2,25,2]        its transformed labels, every LABEL_STEP-th point of each set (the file stays small)
  camera    [C,3,3]           its updated intrinsics"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('DIR_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
OUT = os.path.join(REPO, 'tests', 'golden', 'g25_crop.npz')
sys.path.insert(0, os.path.join(REPO, 'tests', 'helpers'))

# (seed, ratio, size): the reference's own call (0.8, 256) most often, cut_img's default ratio 0.7, ratio 1.0, and a small crop
CASES = [(2500 + i, r, s) for i, (r, s) in enumerate([(0.8, 256)] * 6 + [(0.7, 256)] * 3 + [(1.0, 256)] * 3 + [(0.8, 32), (0.8, 32), (0.7, 32), (1.0, 32)])]


def import_cut_img():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    cv2 = types.ModuleType('cv2')
    cv2.warpAffine = lambda img, M, dsize=None: np.array(M, copy=True)
    sys.modules['cv2'] = cv2
    import dataset.dataset_utils as U
    return U.cut_img


def main():
    import crop_ref as R
    cut_img = import_cut_img()
    rows = {k: [] for k in ('seed', 'ratio', 'size', 'checksum', 'matrix', 'labels', 'camera')}
    for c, (seed, ratio, size) in enumerate(CASES):
        pts, K = R.make_case(seed)
        imgs, labels, cam = cut_img([None], [p.copy() for p in pts], camera=K.copy(), radio=ratio, img_size=size)
        M = imgs[0]
        assert M.dtype == np.float64 and M.shape == (2, 3) and all(l.dtype == np.float64 for l in labels) and cam.dtype == np.float64
        for k, v in zip(('seed', 'ratio', 'size', 'checksum', 'matrix', 'labels', 'camera'),
                        (np.int64(seed), np.float64(ratio), np.int64(size), R.checksum(pts, K), M, np.stack(labels)[:, ::R.LABEL_STEP], cam)):
            rows[k].append(v)
        print('case %2d  seed %d  ratio %.1f  size %3d  s %.6f  t (%.3f, %.3f)' % (c, seed, ratio, size, M[0, 0], M[0, 2], M[1, 2]))
    g = {k: np.stack(v) for k, v in rows.items()}
    np.savez_compressed(OUT, **g)
    print('wrote %s (%d cases, %d arrays, %d bytes)' % (OUT, len(CASES), len(g), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
