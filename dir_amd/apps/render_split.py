"""dataset/prepare_data.py:174-214 (render_data) for the prepared split: <split>/mask/<idx>.jpg and <split>/dense/<idx>.jpg from the
ground-truth MANO meshes of <split>/anno/<idx>.pkl, on the GPU.

    python -m dir_amd.apps.render_split --save_path ROOT --model CKPT --dense_color PKL [--split train] [--bs 256] [--workers N] [--gpu_encode]

Batches of annotations (InterHandSplit.anno) go through gt_batch with the GT layers of the checkpoint (gt_layers_from_checkpoint, which
already carries the fix_shape correction), then the two-hand rasteriser (dir_amd.utils.vis_utils.render_frames, 256 x 256 as IMG_SIZE).
The frames are written as cv.imwrite writes them by default: JPEG quality 95, 4:2:0 chroma subsampling (here through Pillow, on the
same libjpeg), the channels reversed first so that cv.imread / decode_bgr gives back the renderer's array channel order.  Annotation
reads and JPEG encodes run in worker processes, at most 16 of them.  The reference's render_data also makes an empty hms/ folder; it
is made here as well.

--gpu_encode: the JPEG encode is split as the decode of the from-files path is.  The GPU does everything before the Huffman coder
(dir_amd.apps.jpeg.RecordEncoder: colour conversion, 4:2:0 downsampling, forward DCT, quantisation -> one coefficient record per frame);
the worker processes Huffman-code the records and write the files (write_record).  The files are byte-identical to the default path's.
"""
import os
import time

import numpy as np

MAX_WORKERS = 16


def _read_annos(data_path, split, idx):
    from .dataset import InterHandSplit
    ds = InterHandSplit(data_path, split)
    return np.stack([ds.anno(i) for i in idx])


def write_frame(path, frame):
    """one frame in the renderer's array channel order -> JPEG as cv.imwrite(path, frame) writes it (quality 95, 4:2:0)"""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(path, format='JPEG', quality=95, subsampling=2)


def _write(data_path, split, idx, masks, dense):
    for j, i in enumerate(idx):
        write_frame(os.path.join(data_path, split, 'mask', '%d.jpg' % i), masks[j])
        write_frame(os.path.join(data_path, split, 'dense', '%d.jpg' % i), dense[j])
    return len(idx)


def _write_records(data_path, split, idx, masks, dense):
    """--gpu_encode: the workers' half -- coefficient records [n, stride] uint8 -> files"""
    from .jpeg import write_record
    for j, i in enumerate(idx):
        write_record(os.path.join(data_path, split, 'mask', '%d.jpg' % i), masks[j])
        write_record(os.path.join(data_path, split, 'dense', '%d.jpg' % i), dense[j])
    return len(idx)


def default_workers():
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    return max(1, min(MAX_WORKERS, n))


def render_split(data_path, state, dense_color, split='train', bs=256, workers=None, device='cuda', progress=None, gpu_encode=False):
    """render_data(data_path, split) with the GT layers of checkpoint `state` and the dense table `dense_color` (path or [778,3] array)
    -> (images written, seconds).  gpu_encode: everything of the JPEG encode before the Huffman coder runs on the GPU (same files)."""
    import multiprocessing as mp
    import torch
    from .dataset import IMG_SIZE, InterHandSplit, gt_batch, gt_layers_from_checkpoint
    from .. import _capi
    from ..utils import vis_utils as V
    workers = default_workers() if workers is None else max(1, min(MAX_WORKERS, int(workers)))
    mano = gt_layers_from_checkpoint(state, device)
    faces = torch.from_numpy(V.faces_from_layers(mano)).to(device)          # ValueError without th_faces, before anything is written
    colors = torch.from_numpy(V.load_dense_colors(dense_color)).to(device)
    n = len(InterHandSplit(data_path, split))
    for kind in ('mask', 'dense', 'hms'):
        os.makedirs(os.path.join(data_path, split, kind), exist_ok=True)
    ws = torch.empty(int(_capi.lib().dir_render_workspace_bytes(bs)), dtype=torch.uint8, device=device)
    batches = [list(range(s, min(n, s + bs))) for s in range(0, n, bs)]
    chunk = max(1, -(-bs // workers))
    enc = recs = None
    if gpu_encode:
        from .jpeg import RecordEncoder
        enc = RecordEncoder(2 * bs, IMG_SIZE, quality=95, channel_order='bgr')       # the renderer's arrays are what cv.imwrite receives
        recs = torch.empty(2 * bs, enc.record_bytes, dtype=torch.uint8, device=device)
    write = _write_records if gpu_encode else _write
    t0 = time.time()
    done = 0
    with mp.get_context('spawn').Pool(workers) as pool:
        reads = [pool.apply_async(_read_annos, (data_path, split, b)) for b in batches[:2]]
        pending = []
        for k, idx in enumerate(batches):
            an = torch.from_numpy(reads[k].get()).to(device)
            if k + 2 < len(batches):
                reads.append(pool.apply_async(_read_annos, (data_path, split, batches[k + 2])))
            gt = gt_batch(mano, an)
            verts = torch.cat((gt[1], gt[3]), dim=1).contiguous()
            m, d = V.render_frames(verts, faces, gt[8], colors, IMG_SIZE, workspace=ws)
            if gpu_encode:
                nb = len(idx)
                enc(m, recs[:nb], nb)
                enc(d, recs[bs:bs + nb], nb)
                host = recs.cpu().numpy()
                m, d = host[:nb], host[bs:bs + nb]
            else:
                m, d = m.cpu().numpy(), d.cpu().numpy()
            while len(pending) > 2 * workers:                              # bounded: at most ~2 batches of frames in flight
                done += pending.pop(0).get()
            for j in range(0, len(idx), chunk):
                pending.append(pool.apply_async(write, (data_path, split, idx[j:j + chunk], m[j:j + chunk], d[j:j + chunk])))
            if progress:
                progress(done, n)
        for p in pending:
            done += p.get()
    return done, time.time() - t0


def main(argv=None):
    import argparse
    import torch
    ap = argparse.ArgumentParser(description='render_data of dataset/prepare_data.py on MI355X: mask/ and dense/ frames of a prepared split')
    ap.add_argument('--save_path', type=str, required=True, help='the prepared dataset root (<save_path>/<split>/anno/<idx>.pkl)')
    ap.add_argument('--model', type=str, required=True, help='a DIR checkpoint: its MANO buffers give the GT layers and the faces')
    ap.add_argument('--dense_color', type=str, required=True, help="get_dense_color_path()'s pickle ([778,3] in 0..1)")
    ap.add_argument('--split', type=str, default='train', choices=['train', 'val', 'test'])
    ap.add_argument('--bs', type=int, default=256)
    ap.add_argument('--workers', type=int, default=None, help='encode processes (default: the CPUs this process may use, at most 16)')
    ap.add_argument('--gpu_encode', action='store_true', help='JPEG encode split like the decode: DCT + quantisation on the GPU, Huffman coding in the workers (same files)')
    opt = ap.parse_args(argv)
    state = torch.load(opt.model, map_location='cpu', weights_only=False)
    state = state['net'] if isinstance(state, dict) and 'net' in state else state
    from dir_amd.apps import render_split as mod                          # workers pickle the module's functions by this name, not __main__
    n, sec = mod.render_split(opt.save_path, state, opt.dense_color, opt.split, opt.bs, opt.workers, gpu_encode=opt.gpu_encode,
                              progress=lambda k, total: print('\r%d / %d' % (k, total), end='', flush=True))
    print('\n%d images (mask + dense) in %.1f s: %.0f images/s' % (n, sec, n / max(sec, 1e-9)))
    return n


if __name__ == '__main__':
    main()
