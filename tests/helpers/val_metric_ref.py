"""numpy restatement of the validation metric of the reference's training loop (InterHandDataset.evaluate, dataset/interhand.py:262-315)
and the inputs of tests/golden/g24_val_metrics.npz (tools/gen_val_metric_golden.py), which stores seeds and results, not tensors.

  make_case(seed, B, n_stages, exact)   -> (outs_list, targets): float32 numpy arrays, regenerated from numpy.random.RandomState(seed)
  evaluate_np(outs, targets, dtype)     -> (joint L, joint R, vert L, vert R) in mm, the statements of :266-315 in `dtype`
  checksum(outs_list, targets)          -> float64 sum of every input (the fixture stores it: a changed generator is noticed)
"""
import numpy as np

SIDES = ('left', 'right')


def make_case(seed, B, n_stages, exact=False):
    """Two hands 0.8 m from the camera, 12 cm apart.  Predictions live in a frame of their own (shifted, 10 % smaller: root and scale
    matter) with a few mm of error that grows a little from stage to stage; exact=True: predictions equal to the ground truth."""
    rng = np.random.RandomState(seed)
    targets, outs_list = {}, [dict() for _ in range(n_stages)]
    for side, x0 in zip(SIDES, (-0.06, 0.06)):
        c = np.array([x0, 0.0, 0.8])
        j = (c + rng.normal(0, 0.04, (B, 21, 3))).astype(np.float32)
        v = (c + rng.normal(0, 0.05, (B, 778, 3))).astype(np.float32)
        targets['joint_3d_' + side], targets['mesh_3d_' + side] = j, v
        shift = rng.normal(0, 0.1, (B, 1, 3))
        for s in range(n_stages):
            if exact:
                outs_list[s]['pd_joint_xyz_' + side], outs_list[s]['pd_mesh_xyz_' + side] = j.copy(), v.copy()
                continue
            sigma = 0.003 * (1 + 0.25 * s)
            outs_list[s]['pd_joint_xyz_' + side] = ((j - c) / 1.1 + shift + rng.normal(0, sigma, j.shape)).astype(np.float32)
            outs_list[s]['pd_mesh_xyz_' + side] = ((v - c) / 1.1 + shift + rng.normal(0, sigma, v.shape)).astype(np.float32)
    return outs_list, targets


def checksum(outs_list, targets):
    t = sum(float(np.sum(v, dtype=np.float64)) for _, v in sorted(targets.items()))
    return t + sum(float(np.sum(v, dtype=np.float64)) for o in outs_list for _, v in sorted(o.items()))


def evaluate_np(outs, targets, dtype=np.float64):
    """interhand.py:266-315 for one stage's outputs; `dtype` is the precision of every operation (the mean included, as numpy's .mean()
    of an array of that dtype).  -> [joint L, joint R, vert L, vert R] (mm), an array of `dtype`"""
    res = {}
    for side in SIDES:
        jg, vg = np.asarray(targets['joint_3d_' + side], dtype), np.asarray(targets['mesh_3d_' + side], dtype)
        jp, vp = np.asarray(outs['pd_joint_xyz_' + side], dtype), np.asarray(outs['pd_mesh_xyz_' + side], dtype)
        root_g, root_p = jg[:, 9:10], jp[:, 9:10]
        len_g = np.linalg.norm(jg[:, 9] - jg[:, 0], axis=-1)
        len_p = np.linalg.norm(jp[:, 9] - jp[:, 0], axis=-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            scale = (len_g / len_p)[:, None, None]
            res['j' + side] = np.linalg.norm((jp - root_p) * scale - (jg - root_g), axis=-1).mean() * 1000
            res['v' + side] = np.linalg.norm((vp - root_p) * scale - (vg - root_g), axis=-1).mean() * 1000
    return np.array([res['jleft'], res['jright'], res['vleft'], res['vright']], dtype)


def fixture_cases(g):
    """the fixture's cases as dicts: seed, B, n_stages, exact, ref32 [n_stages,4] float32, ref64 [n_stages,4] float64, checksum"""
    out = []
    for c in range(int(g['cases'])):
        out.append({'seed': int(g['seed.%d' % c]), 'B': int(g['B.%d' % c]), 'n_stages': int(g['n_stages.%d' % c]),
                    'exact': bool(g['exact.%d' % c]), 'ref32': g['ref32.%d' % c], 'ref64': g['ref64.%d' % c],
                    'checksum': float(g['checksum.%d' % c])})
    return out


def fixture_d(cases):
    """the reference's own float32 error: the largest |ref32 - ref64| (mm) over the fixture"""
    return max(float(np.max(np.abs(c['ref32'].astype(np.float64) - c['ref64']))) for c in cases)
