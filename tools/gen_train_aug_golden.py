"""Writes tests/golden/g23_train_aug.npz: the label side and the seg rule of dataset/interhand.py:__getitem__ (split 'train'), computed
by the REFERENCE's own code on the CPU.  Authoring only: it imports the reference tree (path: $DIR_REFERENCE, default ../reference next to
the repository), which never travels with the tests.  cv2, imgaug and yacs are stubbed: the functions run here (get_affine_mat, flip and
data_augmentation_3D with img_list=None, uvd2xyz_np) never call them.

  python tools/gen_train_aug_golden.py

One set of inputs, shared by every case (the fixture stays small):
  in.*      float32: camera-space joints [21,3] / verts [778,3] of both hands, their uv (the gt_batch outputs), camera K
  the seg mask is not stored: uint8 [256,256,3] with B = 0, G = x and R = y (`seg_mask()`), every (G, R) pair once, ties and both sides of
            the threshold 50 included
  vsub      the vertex rows whose targets are stored (every 26th and the last; the per-point maths is the same for every row)
Per case c (16 parameter sets: rot +-180, scale 0.9 / 1.1, tx, ty +-10, flips):
  M.c       get_affine_mat(rot, scale, tx, ty, 256, 256) (float32 [3,3]);  flip.c, rot.c, scale.c, tx.c, ty.c
  out.c.*   the 8 targets (mesh_*: rows vsub only) + center_left / center_right, float64, by the statements of interhand.py:170-240
            on the float64 inputs
  seg.c     (c = 0, 1: without / with flip) the seg of interhand.py:206-216 (extracted from the file) on seg_mask(), uint8"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('DIR_REFERENCE', os.path.join(os.path.dirname(REPO), 'reference'))
OUT = os.path.join(REPO, 'tests', 'golden', 'g23_train_aug.npz')


def import_ref_utils():
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
    import utils.utils as U
    return U


def seg_statements():
    """interhand.py's seg block, from `seg = np.zeros` to `seg = seg[np.newaxis, :, :]`, as source text"""
    lines = open(os.path.join(REF, 'dataset', 'interhand.py')).read().split('\n')
    i0 = next(i for i, l in enumerate(lines) if l.strip().startswith('seg = np.zeros'))
    i1 = next(i for i, l in enumerate(lines) if l.strip().startswith('seg = seg[np.newaxis'))
    block = lines[i0:i1 + 1]
    ind = len(block[0]) - len(block[0].lstrip())
    return '\n'.join(l[ind:] for l in block)


def seg_mask():
    """B = 0, G = x, R = y"""
    mask = np.zeros((256, 256, 3), np.uint8)
    mask[..., 1] = np.arange(256, dtype=np.uint8)[None, :]
    mask[..., 2] = np.arange(256, dtype=np.uint8)[:, None]
    return mask


def main():
    U = import_ref_utils()
    imgUtils = U.imgUtils
    rng = np.random.RandomState(23)
    B = 16
    cases = [(180.0, 1.0, 0.0, 0.0, False), (-180.0, 1.0, 0.0, 0.0, True), (0.0, 0.9, 0.0, 0.0, False), (0.0, 1.1, 0.0, 0.0, True),
             (0.0, 1.0, 10.0, -10.0, False), (0.0, 1.0, -10.0, 10.0, True), (90.0, 1.1, 10.0, 10.0, True), (-90.0, 0.9, -10.0, -10.0, False),
             (0.0, 1.0, 0.0, 0.0, True), (0.0, 1.0, 0.0, 0.0, False)]
    while len(cases) < B:
        cases.append((float(rng.uniform(-180, 180)), float(1 + rng.uniform(-0.1, 0.1)), float(rng.uniform(-10, 10)), float(rng.uniform(-10, 10)),
                      bool(rng.rand() < 0.5)))
    g = {}
    seg_src = seg_statements()
    mask = seg_mask()
    vsub = np.r_[0:778:26, 777]
    g['vsub'] = vsub
    K = np.array([[1503.5, 0, 129.25], [0, 1491.0, 125.5], [0, 0, 1]], np.float32)
    for side, x0 in (('left', -0.06), ('right', 0.06)):
        j = (np.array([x0, 0.0, 0.8]) + rng.normal(0, 0.04, (21, 3))).astype(np.float32)
        v = (np.array([x0, 0.0, 0.8]) + rng.normal(0, 0.05, (778, 3))).astype(np.float32)
        for nm, a in (('joint', j), ('mesh', v)):
            p = a.astype(np.float64) @ K.astype(np.float64).T
            g['in.%s_xyz_%s' % (nm, side)] = a
            g['in.%s_uv_%s' % (nm, side)] = (p[:, :2] / p[:, 2:]).astype(np.float32)
    g['in.camera'] = K
    for c, (rot, scale, tx, ty, flip) in enumerate(cases):
        d = lambda k: g['in.%s' % k].astype(np.float64)  # noqa: E731
        handJ_left, handV_left, handJ_right, handV_right = d('joint_xyz_left'), d('mesh_xyz_left'), d('joint_xyz_right'), d('mesh_xyz_right')
        handJ2d_left_uv, handV2d_left_uv = d('joint_uv_left'), d('mesh_uv_left')
        handJ2d_right_uv, handV2d_right_uv = d('joint_uv_right'), d('mesh_uv_right')
        camera = K.astype(np.float64)
        # interhand.py:168-200, the label statements, with img_list=None
        if flip:
            _, label2d_list = imgUtils.flip(None, [handJ2d_left_uv, handJ2d_right_uv, handV2d_left_uv, handV2d_right_uv], 256)
            handJ2d_right_uv, handJ2d_left_uv, handV2d_right_uv, handV2d_left_uv = label2d_list
            handJ_right, handJ_left, handV_right, handV_left = handJ_left, handJ_right, handV_left, handV_right
        _, label2d_list, label3d_list, _ = imgUtils.data_augmentation_3D(
            rot, scale, tx, ty, camera, None, [handJ2d_left_uv, handJ2d_right_uv, handV2d_left_uv, handV2d_right_uv],
            [handJ_left[:, 2:], handJ_right[:, 2:], handV_left[:, 2:], handV_right[:, 2:]], img_size=256)
        handJ2d_left_uv, handJ2d_right_uv, handV2d_left_uv, handV2d_right_uv = label2d_list
        handJ_left, handJ_right, handV_left, handV_right = label3d_list
        g['out.%d.center_left' % c] = handJ_left[9:10].copy()
        g['out.%d.center_right' % c] = handJ_right[9:10].copy()
        g['out.%d.joint_2d_left' % c] = np.concatenate((handJ2d_left_uv / 256 * 2 - 1, handJ_left[:, 2:]), axis=-1)
        g['out.%d.joint_2d_right' % c] = np.concatenate((handJ2d_right_uv / 256 * 2 - 1, handJ_right[:, 2:]), axis=-1)
        g['out.%d.mesh_2d_left' % c] = np.concatenate((handV2d_left_uv / 256 * 2 - 1, handV_left[:, 2:]), axis=-1)[vsub]
        g['out.%d.mesh_2d_right' % c] = np.concatenate((handV2d_right_uv / 256 * 2 - 1, handV_right[:, 2:]), axis=-1)[vsub]
        g['out.%d.joint_3d_left' % c], g['out.%d.mesh_3d_left' % c] = handJ_left, handV_left[vsub]
        g['out.%d.joint_3d_right' % c], g['out.%d.mesh_3d_right' % c] = handJ_right, handV_right[vsub]
        g['M.%d' % c] = imgUtils.get_affine_mat(theta=rot, scale=scale, u=tx, v=ty, height=256, width=256)
        g['flip.%d' % c], g['rot.%d' % c], g['scale.%d' % c], g['tx.%d' % c], g['ty.%d' % c] = flip, rot, scale, tx, ty
        if c < 2:
            ns = {'np': np, 'mask': mask, 'do_flip': flip, 'self': types.SimpleNamespace(img_size=256)}
            exec(seg_src, ns)
            g['seg.%d' % c] = ns['seg'].astype(np.uint8)
    g['cases'] = np.int64(B)
    np.savez_compressed(OUT, **g)
    print('wrote %s (%d cases, %d arrays)' % (OUT, B, len(g)))


if __name__ == '__main__':
    main()
