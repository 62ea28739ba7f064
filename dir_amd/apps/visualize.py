"""Pictures of what the network predicts: the two predicted hand meshes, Phong-shaded, drawn over the input frames.

    python -m dir_amd.apps.visualize --model CKPT --data_path ROOT [--split test] --out DIR [--num 64] [--bs 32] [--stage 2]
                                     [--dtype f16] [--joints]

Frames come from the prepared split through dataset.DecodeRing (<split>/img/<idx>.jpg, decoded to the uint8 BGR frames the network sees);
each batch is one DirEngine.forward, then dir_amd.utils.vis_utils.overlay_predictions on stage `--stage` of its output (0 = the initial
regression, 1 and 2 = the two refinement stages; 2 is the final prediction), rendered over the frames in one launch.  <out>/<idx>.png is
the frame and the overlay side by side, written with Pillow (PNG: lossless), in RGB.  With --joints the predicted 2-D joints and bones of
that stage are drawn on top (vis_utils.draw_joints: this project's own coverage rule and palette, not OpenCV's drawing).
"""
import os
import time

import numpy as np


def write_png(path, frame_bgr, overlay_bgr):
    """frame | overlay side by side, BGR uint8 [S,S,3] each -> an RGB PNG"""
    from PIL import Image
    both = np.concatenate([frame_bgr, overlay_bgr], axis=1)[:, :, ::-1]
    Image.fromarray(np.ascontiguousarray(both)).save(path, format='PNG')


def visualize(eng, renderer, data_path, out_dir, split='test', num=64, bs=32, stage=2, workers=4, joints=False, indices=None):
    """-> (images written, seconds).  `eng`: a DirEngine; `renderer`: a mano_two_hands_shaded_renderer of the network's input size."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from ..utils import vis_utils as V
    from .dataset import IMG_SIZE, DecodeRing, InterHandSplit
    if renderer.img_size != IMG_SIZE:
        raise ValueError('visualize: the renderer must draw %d x %d pictures, the size of the frames' % (IMG_SIZE, IMG_SIZE))
    if indices is None:
        indices = list(range(min(int(num), len(InterHandSplit(data_path, split)))))
    os.makedirs(out_dir, exist_ok=True)
    dev = eng.device
    ring = DecodeRing(data_path, split, bs, workers=max(1, min(int(workers), 16)), indices=indices)
    done, t0 = 0, time.perf_counter()
    try:
        with ThreadPoolExecutor(max_workers=8) as pool:
            jobs = []
            for k, (frames, _, n) in enumerate(ring):
                f = frames[:n].to(dev).contiguous()
                outs = eng.forward(f, want_proj_feat=False)
                over = V.overlay_predictions(outs[stage], f, renderer)
                if joints:
                    over = V.draw_joints(over, outs[stage]['pd_joint_uv_left'], outs[stage]['pd_joint_uv_right'])
                fh, oh = f.cpu().numpy(), over.cpu().numpy()
                for j in range(n):
                    jobs.append(pool.submit(write_png, os.path.join(out_dir, '%d.png' % indices[k * bs + j]), fh[j], oh[j]))
            for j in jobs:
                j.result()
                done += 1
    finally:
        ring.close()
    return done, time.perf_counter() - t0


def main(argv=None):
    import argparse

    import torch

    from ..engine import DirEngine
    from ..utils import vis_utils as V
    from .dataset import IMG_SIZE, gt_layers_from_checkpoint
    ap = argparse.ArgumentParser(description='draw the predicted two-hand meshes of a DIR checkpoint over the frames of a prepared split')
    ap.add_argument('--model', type=str, required=True)
    ap.add_argument('--ema', action='store_true', help="load the averaged weights (the checkpoint's 'ema' key, written by dir_amd.apps.train --ema_decay) instead of 'net'")
    ap.add_argument('--data_path', type=str, required=True)
    ap.add_argument('--split', type=str, default='test', choices=['train', 'val', 'test'])
    ap.add_argument('--out', type=str, required=True)
    ap.add_argument('--num', type=int, default=64, help='the first NUM images of the split')
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--stage', type=int, default=2, choices=[0, 1, 2], help='0: the initial regression, 1 / 2: the refinement stages (2 = final)')
    ap.add_argument('--dtype', choices=['f16', 'bf16', 'f32'], default='f16')
    ap.add_argument('--workers', type=int, default=4, help='decode processes')
    ap.add_argument('--joints', action='store_true', help='draw the predicted 2-D joints on the overlay')
    opt = ap.parse_args(argv)
    state = torch.load(opt.model, map_location='cpu', weights_only=False)
    from . import checkpoint_weights
    state = checkpoint_weights(state, opt.ema, opt.model)
    eng = DirEngine(state, dtype={'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[opt.dtype], root_joint=0)
    mano = gt_layers_from_checkpoint(state)
    # the dense table only feeds render_densepose, which is not used here
    renderer = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((V.NV_HAND, 3)), img_size=IMG_SIZE,
                                                device=eng.device)
    n, sec = visualize(eng, renderer, opt.data_path, opt.out, opt.split, opt.num, opt.bs, opt.stage, opt.workers, opt.joints)
    print('%d pictures in %.1f s: %.0f images/s' % (n, sec, n / max(sec, 1e-9)))
    return n


if __name__ == '__main__':
    main()
