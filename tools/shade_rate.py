"""Times of the shaded / orthographic renderer next to the existing rasteriser, and of the visualize tool.

  python tools/shade_rate.py [--bs 32] [--size 256] [--rounds 7] [--vis_n 0] [--out FILE]

One process, warmed, HIP events, the variants alternating within every round, on the ground-truth meshes of the fake train split
(tests/helpers/fake_train_split.py: synthetic random faces, the worst case README.md names):
  plain    dir_render_two_hands writing color_f32 (the existing entry point; its instantiation is unchanged)
  shaded   vertex normals + the shaded orthographic render writing shaded_f32 (dir_render_shaded)
  overlay  the same writing overlay_u8 over uint8 frames
Per variant: the median over the rounds and the spread (min .. max), in ms per batch.  With --vis_n N also dir_amd.apps.visualize over a
fake N-image test split with synthetic weights, images/s end to end."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests', 'helpers')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--vis_n', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fake_train_split import write_train_split
    from dir_amd import synth
    from dir_amd.apps import dataset as DS
    from dir_amd.utils import vis_utils as V
    with open(os.path.join(REPO, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}
    mano = DS.gt_layers_from_checkpoint(sd)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    B, S = a.bs, a.size
    with tempfile.TemporaryDirectory() as d:
        write_train_split(d, B, seed=3)
        ds = DS.InterHandSplit(d, 'train')
        gt = DS.gt_batch(mano, torch.from_numpy(np.stack([ds.anno(i) for i in range(B)])).cuda())
    verts, K = torch.cat((gt[1], gt[3]), 1).contiguous(), gt[8].contiguous()
    xy = verts[..., :2]
    lo, hi = xy.min(1).values, xy.max(1).values
    scale = (0.8 / (hi - lo).max(-1).values).contiguous()
    trans = (-2 * scale[:, None] * (lo + hi) / 2).contiguous()
    colors = torch.from_numpy(V.default_colors()).cuda()
    frames = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device='cuda')
    ws0 = torch.empty(int(V._capi.lib().dir_render_workspace_bytes(B)), dtype=torch.uint8, device='cuda')
    ws1 = torch.empty(int(V._capi.lib().dir_render_shaded_workspace_bytes(B)), dtype=torch.uint8, device='cuda')
    variants = {
        'plain': lambda: V.rasterize(verts, faces, K, S, colors=colors, outputs=('color_f32',), workspace=ws0),
        'shaded': lambda: V.rasterize_shaded(verts, faces, S, colors=colors, scale=scale, trans2d=trans, outputs=('shaded_f32',), workspace=ws1),
        'overlay': lambda: V.rasterize_shaded(verts, faces, S, colors=colors, scale=scale, trans2d=trans, background=frames,
                                              outputs=('overlay_u8',), workspace=ws1),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)
    cov = float((variants['shaded']()['shaded_f32'] != variants['shaded']()['shaded_f32'][0, 0, 0, 0]).any(-1).float().mean())
    res = {'B': B, 'size': S, 'rounds': a.rounds, 'reps': a.reps, 'covered_ortho': cov,
           'ms_per_batch': {k: {'median': float(np.median(v)), 'min': min(v), 'max': max(v)} for k, v in ms.items()}}
    if a.vis_n:
        from fake_split import write_split
        from dir_amd.apps import visualize as VZ
        from dir_amd.engine import DirEngine
        eng = DirEngine(sd, dtype=torch.float16)
        r = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((778, 3)), img_size=256, device='cuda')
        with tempfile.TemporaryDirectory() as d:
            write_split(os.path.join(d, 'data'), a.vis_n, seed=0)
            VZ.visualize(eng, r, os.path.join(d, 'data'), os.path.join(d, 'warm'), num=min(a.vis_n, 32), bs=32, workers=8)
            n, sec = VZ.visualize(eng, r, os.path.join(d, 'data'), os.path.join(d, 'out'), num=a.vis_n, bs=32, workers=8)
        res['visualize'] = {'images': n, 'seconds': sec, 'images_per_sec': n / sec}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
