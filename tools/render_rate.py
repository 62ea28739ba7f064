"""Rate of the two-hand rasteriser (csrc/render.hip) and of the render_split tool.

  python tools/render_rate.py [--bs 32,256] [--size 256] [--split_n 0] [--workers 16] [--out FILE]

GPU time per batch of render_frames (mask + dense, HIP events) on the ground-truth meshes of synthetic annotations with the synthetic
GT layers; with --split_n N also render_split over a fake N-image train split (tests/helpers/fake_train_split.py), images/s end to end
(annotation reads, GT MANO, render, JPEG encodes by --workers processes)."""
import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests', 'helpers')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', default='32,256')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--split_n', type=int, default=0)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from dir_amd import synth
    from dir_amd.apps import dataset as DS
    from dir_amd.utils import vis_utils as V
    with open(os.path.join(REPO, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items() if 'mano_layer' in k}
    mano = DS.gt_layers_from_checkpoint(sd)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    table = np.random.default_rng(0).random((778, 3))
    colors = torch.from_numpy(V.load_dense_colors(table)).cuda()
    res = {'size': a.size}
    for B in [int(b) for b in a.bs.split(',')]:
        g = torch.Generator().manual_seed(B)
        an = torch.zeros(B, DS.ANNO_FLOATS)
        an[:, 0:9] = torch.eye(3).reshape(9)
        an[:, 9:12] = torch.tensor([0.0, 0.0, 0.8]) + 0.02 * torch.randn(B, 3, generator=g)
        an[:, 12:21] = torch.tensor([[1500., 0, 128], [0, 1500, 128], [0, 0, 1]]).reshape(9)
        for h in range(2):
            an[:, 21 + 67 * h:30 + 67 * h] = torch.eye(3).reshape(9)
            an[:, 30 + 67 * h:75 + 67 * h] = 0.5 * torch.randn(B, 45, generator=g)
            an[:, 85 + 67 * h:88 + 67 * h] = torch.tensor([-0.06 if h == 0 else 0.06, 0.0, 0.0])
        gt = DS.gt_batch(mano, an.cuda())
        verts = torch.cat((gt[1], gt[3]), 1).contiguous()
        ws = torch.empty(int(V._capi.lib().dir_render_workspace_bytes(B)), dtype=torch.uint8, device='cuda')
        for _ in range(3):
            m, d = V.render_frames(verts, faces, gt[8], colors, a.size, workspace=ws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            V.render_frames(verts, faces, gt[8], colors, a.size, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        res['B%d' % B] = {'ms_per_batch': ms, 'images_per_sec': B / ms * 1e3, 'covered': float((m != 1).any(-1).float().mean())}
    if a.split_n:
        from fake_train_split import write_train_split
        from dir_amd.apps.render_split import render_split
        with tempfile.TemporaryDirectory() as d:
            write_train_split(d, a.split_n, seed=0)
            pk = os.path.join(d, 'dense.pkl')
            with open(pk, 'wb') as f:
                pickle.dump(table, f)
            n, sec = render_split(d, sd, pk, 'train', bs=256, workers=a.workers)
        res['render_split'] = {'images': n, 'seconds': sec, 'images_per_sec': n / sec, 'workers': a.workers}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
