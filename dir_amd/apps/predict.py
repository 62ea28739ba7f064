"""The network on your own photos or a video: full-size frames of any size -> the crop the network was trained on (dir_amd.utils.crop, on
the GPU) -> DirEngine.forward -> predictions in FRAME pixels.

    python -m dir_amd.apps.predict --model CKPT --input DIR|FILES --out DIR [--boxes boxes.json] [--track] [--ratio 0.8] [--bs 32]
                                   [--stage 2] [--dtype f16|bf16|f32] [--workers 8] [--pictures] [--joints] [--obj] [--antialias]

Input: image files (jpg / jpeg / png / bmp) in natural name order, decoded to BGR on the host with Pillow by worker threads that never
touch the GPU, packed into FrameBatches of at most --bs images.  --boxes: a JSON object {"name": [x0, y0, x1, y1]} keyed by file name (or
stem): the tight box around both hands in frame pixel positions; an image without an entry uses the whole frame (0, 0, W - 1, H - 1).
The hands are expected to fill --ratio of the crop (the reference prepares its data with 0.8).

Without --track every image is independent: boxes -> matrices -> crops -> forward.  With --track the input is a sequence (or, when it
has sub-directories, one sequence per sub-directory, advancing in lockstep, one frame each per forward; more than --bs sub-directories
walk --bs at a time): frame 0 takes its box from --boxes (there "sequence/name" or "sequence/stem" comes before the bare name, so that
a/0.png and b/0.png may start from different boxes) or the whole frame, frame t + 1 the box of frame t's predicted meshes (crop_matrices_from_meshes of stage --stage), chained on the
device with no host read between frames.  Where a prediction gives no usable box the previous one holds: "tracked": false.

--antialias: a crop that shrinks the frame (a hand box larger than 256 px, as in a 1080p or 4K photo) is resampled with a triangle filter
as wide as the shrink (crop_frames(antialias=True): Pillow's resize(BILINEAR, box)) instead of four taps per pixel, which skip most of the
frame's pixels and alias; a crop that does not shrink is unchanged.  The matrices, and with them the way back to frame pixels, are the same.

Output per image, <out>/<stem>.json (in --track with sub-directories <out>/<sequence>/<stem>.json):
  image, width, height   the file and its size
  box                    the tight box the crop was made from (null for a frame whose crop was tracked or held)
  matrix                 the 2x3 crop matrix (crop position = matrix * frame position), doubles
  valid                  false: no crop could be made (the crop is black, the numbers below are not finite and written as null)
  tracked                true: the matrix comes from the previous frame's prediction
  left / right           joints_px [21][2] frame pixels, joints_xyz [21][3] metres (root-relative), camera_px {"scale", "trans"}: frame
                         pixel = scale * xy + trans for this hand's vertices and joints
  offset                 the predicted offset between the hands' roots (pd_offset)
  antialiased            only with --antialias: true where the crop was made with the anti-aliased rule (it shrinks the frame)
--pictures: <stem>.png, crop | overlay side by side as apps.visualize writes them (--joints as there).  --obj: <stem>.obj, both hands
placed as vis_utils.prediction_camera places them, faces from the checkpoint.  The last line printed is "N images in T s: R images/s".
"""
import json
import os
import re
import time

import numpy as np

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')
SIZE = 256                     # the network's input (dataset.IMG_SIZE)
SIDES = ('left', 'right')


def _natural(path):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r'(\d+)', os.path.basename(path))]


def list_images(inputs):
    """files and / or directories -> the image files among them, in natural name order (f2 before f10)"""
    out = []
    for p in inputs:
        if os.path.isdir(p):
            out += [os.path.join(p, n) for n in os.listdir(p) if n.lower().endswith(EXTENSIONS) and os.path.isfile(os.path.join(p, n))]
        elif p.lower().endswith(EXTENSIONS):
            out.append(p)
        else:
            raise ValueError('predict: %s is neither a directory nor a %s file' % (p, ' / '.join(EXTENSIONS)))
    return sorted(out, key=_natural)


def list_sequences(inputs):
    """--track: one directory with sub-directories -> one sequence per sub-directory (natural order); anything else -> one sequence"""
    if len(inputs) == 1 and os.path.isdir(inputs[0]):
        subs = sorted((os.path.join(inputs[0], n) for n in os.listdir(inputs[0]) if os.path.isdir(os.path.join(inputs[0], n))), key=_natural)
        seqs = [s for s in (list_images([d]) for d in subs) if s]
        if seqs:
            return seqs
    return [list_images(inputs)]


def decode_bgr(path):
    """an image file -> uint8 BGR [H,W,3] (Pillow; host only)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def box_for(boxes, path, height, width):
    """the entry of --boxes for a file, or the whole frame.  Keys, in this order: directory/name, directory/stem (the file's own directory,
    which is the sequence's name in --track with sub-directories, so that a/0.png and b/0.png may differ), then name, then stem"""
    name = os.path.basename(path)
    stem, seq = os.path.splitext(name)[0], os.path.basename(os.path.dirname(os.path.abspath(path)))
    for k in (seq + '/' + name, seq + '/' + stem, name, stem):
        if boxes and k in boxes:
            b = [float(v) for v in boxes[k]]
            if len(b) != 4:
                raise ValueError('predict: the box of %s must be [x0, y0, x1, y1]' % k)
            return b
    return [0.0, 0.0, float(width - 1), float(height - 1)]


class Tracker(object):
    """The crop of every frame of one or more sequences that advance in lockstep.

        tr = Tracker(eng, ratio=0.8, stage=2)
        crops, outs = tr.step(FrameBatch(frames_t), boxes_t0)     # boxes: [B,4] for the first step (None: whole frames), ignored afterwards

    A later step may bring fewer frames than the one before: the sequences at the tail of the batch have ended.  With track=False every
    step is a first step.

    After a step: `M` float64 [B,6] the matrices the crops were made with, `valid` int32 [B] whether a crop could be made, `tracked`
    int32 [B] whether the matrix came from the previous prediction (0 on the first step and where the box was held); all on the
    device.  The next matrices are made right after the forward, on the device, with no host read.  With antialias=True the crops are
    crop_frames(antialias=True) and `area` int32 [B] says which of them got the anti-aliased rule (None otherwise)."""

    def __init__(self, eng, ratio=0.8, stage=2, size=SIZE, track=True, antialias=False):
        self.eng, self.ratio, self.stage, self.size, self.track = eng, float(ratio), int(stage), int(size), bool(track)
        self.antialias = bool(antialias)
        self.M = self.valid = self.tracked = self.area = None
        self._next = None

    def step(self, batch, boxes=None):
        import torch

        from ..utils import crop as CR
        dev, B = self.eng.device, len(batch)
        if self._next is None or not self.track:
            if boxes is None:
                boxes = [[0.0, 0.0, w - 1.0, h - 1.0] for h, w in batch.sizes]
            b = torch.as_tensor(np.asarray(boxes, np.float32).reshape(B, 4)).to(dev)
            self.M, self.valid = CR.crop_matrices_from_boxes(b, self.ratio, self.size)
            self.tracked = torch.zeros(B, dtype=torch.int32, device=dev)
        else:
            if self._next[0].shape[0] < B:
                raise ValueError('Tracker.step: %d frames after %d: sequences may end (from the tail of the batch), not begin' % (B, self._next[0].shape[0]))
            M, ok, prev_valid = (x[:B].contiguous() for x in self._next)
            # a held box is as good as it was: the crop stays valid where the previous one was
            self.M, self.tracked, self.valid = M, ok, torch.maximum(ok, prev_valid)
        if self.antialias:
            crops, status, self.area = CR.crop_frames(batch, self.M, self.valid, self.size, return_status=True, antialias=True, return_area=True)
        else:
            crops, status = CR.crop_frames(batch, self.M, self.valid, self.size, return_status=True)
        self.valid = self.valid * (status == 0).to(torch.int32)            # a crop the kernel refused is black: the image is not valid
        outs = self.eng.forward(crops, want_proj_feat=False)
        if self.track:
            self._next = CR.crop_matrices_from_meshes(outs[self.stage], self.M, self.ratio, self.size) + (self.valid,)
        return crops, outs


def _records(paths, batch, boxes_used, tr, outs, stage, keep_stage):
    """one host read per batch -> the JSON records of its images"""
    from ..utils import crop as CR
    o = outs[stage]
    M = tr.M
    t = {'M': M, 'valid': tr.valid, 'tracked': tr.tracked, 'offset': o['pd_offset'].float()}
    if tr.area is not None:
        t['area'] = tr.area
    for s in SIDES:
        t['px_' + s] = CR.to_frame_pixels(o['pd_joint_uv_' + s].float(), M, tr.size)
        t['xyz_' + s] = o['pd_joint_xyz_' + s].float()
        t['sc_' + s], t['tr_' + s] = CR.frame_camera(o['pd_proj_' + s].float(), M, tr.size)
    if keep_stage:
        for k in ('pd_mesh_xyz_left', 'pd_mesh_xyz_right', 'pd_proj_left', 'pd_proj_right', 'pd_joint_uv_left', 'pd_joint_uv_right'):
            t[k] = o[k].float()
    h = {k: v.cpu().numpy() for k, v in t.items()}

    def num(a):
        return [num(x) for x in a] if isinstance(a, (list, tuple)) else (a if np.isfinite(a) else None)
    recs = []
    for j, p in enumerate(paths):
        first = not h['tracked'][j] and boxes_used is not None
        r = {'image': os.path.basename(p), 'width': int(batch.sizes[j][1]), 'height': int(batch.sizes[j][0]),
             'box': [float(v) for v in boxes_used[j]] if first else None, 'matrix': h['M'][j].reshape(2, 3).tolist(),
             'valid': bool(h['valid'][j]), 'tracked': bool(h['tracked'][j])}
        for s in SIDES:
            r[s] = {'joints_px': num(h['px_' + s][j].tolist()), 'joints_xyz': num(h['xyz_' + s][j].tolist()),
                    'camera_px': {'scale': num(float(h['sc_' + s][j])), 'trans': num(h['tr_' + s][j].tolist())}}
        r['offset'] = num(h['offset'][j].reshape(-1).tolist())
        if 'area' in h:
            r['antialiased'] = bool(h['area'][j])
        if keep_stage:
            r['stage'] = {k: h[k][j] for k in h if k.startswith('pd_')}
        recs.append(r)
    return recs


def write_obj(path, verts, faces):
    """verts [1556,3] (both hands in one frame), faces int [3076,3] (0-based) -> a Wavefront OBJ"""
    with open(path, 'w') as f:
        f.write('# left hand: vertices 1..778, right hand: 779..1556\n')
        f.write(''.join('v %.6f %.6f %.6f\n' % tuple(v) for v in verts.tolist()))
        f.write(''.join('f %d %d %d\n' % (a + 1, b + 1, c + 1) for a, b, c in faces.tolist()))


def lockstep(seqs):
    """sequences -> the steps of their lockstep walk: step t holds (sequence index, item t) of every sequence that has one, the longest
    sequence first, so that a sequence that ends leaves from the tail of the batch"""
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), i))
    return [[(i, seqs[i][t]) for i in order if len(seqs[i]) > t] for t in range(len(seqs[order[0]]) if seqs else 0)]


def lockstep_groups(seqs, bs):
    """more sequences than `bs`: `bs` of them walk in lockstep at a time, one group after the other, so that no batch exceeds `bs`
    -> per group the steps of lockstep(), with the sequences' indices in `seqs`"""
    return [[[(g0 + i, item) for i, item in st] for st in lockstep(seqs[g0:g0 + bs])] for g0 in range(0, len(seqs), bs)]


def _walk(eng, steps, load, names, box_of, ratio, stage, track, keep_stage, antialias=False):
    """the one loop: per step FrameBatch -> Tracker.step -> records.  load(k) -> the decoded frames of step k; box_of(entry, h, w) -> the
    box of a step entry.  Yields (entries, records, crops, outs) with the device tensors of that step."""
    from ..utils import crop as CR
    tr = Tracker(eng, ratio, stage, track=track, antialias=antialias)
    for k, st in enumerate(steps):
        batch = CR.FrameBatch(load(k))
        used = [box_of(e, h, w) for e, (h, w) in zip(st, batch.sizes)] if (not track or k == 0) else None
        crops, outs = tr.step(batch, used)
        yield st, _records([names(e) for e in st], batch, used, tr, outs, stage, keep_stage), crops, outs


def predict(eng, frames, boxes=None, ratio=0.8, stage=2, bs=32, track=False, keep_stage=False, keep_crops=False, antialias=False):
    """The loop behind the command, on decoded frames.

    frames: without `track` a list of uint8 BGR arrays [H,W,3] of any sizes, taken `bs` at a time; with `track` a list of sequences (each
    a list of frames), advanced in lockstep -- one frame of every sequence per forward, a shorter sequence dropping out at its end; more
    than `bs` sequences walk `bs` at a time, one group after the other.
    boxes: one (x0, y0, x1, y1) or None per image (with `track` per sequence: the box of its frame 0); None: whole frames.
    -> a list of records (the JSON fields; with `track` one list per sequence), each with 'crop' (uint8 [256,256,3]) when keep_crops and
    'stage' (the stage's meshes, projections and joint uv as numpy arrays) when keep_stage.  antialias: anti-aliased crops where a crop
    shrinks its frame; every record then has 'antialiased'."""
    if track:
        groups = lockstep_groups([list(s) for s in frames], bs)
        out = [[] for _ in frames]
    else:
        groups = [[[(i, frames[i]) for i in range(b0, min(b0 + bs, len(frames)))] for b0 in range(0, len(frames), bs)]]
        out = [None] * len(frames)

    def box_of(e, h, w):
        return [float(v) for v in boxes[e[0]]] if boxes is not None and boxes[e[0]] is not None else [0.0, 0.0, w - 1.0, h - 1.0]
    for steps in groups:
        for st, recs, crops, outs in _walk(eng, steps, lambda k: [f for _, f in steps[k]], lambda e: str(e[0]), box_of, ratio, stage, track, keep_stage,
                                            antialias):
            ch = crops.cpu().numpy() if keep_crops else None
            for j, ((i, _), r) in enumerate(zip(st, recs)):
                if keep_crops:
                    r['crop'] = ch[j]
                if track:
                    out[i].append(r)
                else:
                    out[i] = r
    return out


def run(eng, sequences, out_dir, boxes=None, ratio=0.8, stage=2, bs=32, track=False, workers=8, pictures=False, joints=False, obj=False,
        renderer=None, faces=None, antialias=False):
    """files -> files.  sequences: [[paths]] (one list without `track`).  -> (images, seconds, seconds of them spent waiting for decoded
    frames).  Two steps are decoded ahead of the GPU by at most 16 threads; the files are written by 8 more.  With `track`, more than `bs`
    sequences walk `bs` at a time, so that no batch holds more than `bs` images."""
    from concurrent.futures import ThreadPoolExecutor

    from ..utils import vis_utils as V
    from .visualize import write_png
    os.makedirs(out_dir, exist_ok=True)
    named = track and len(sequences) > 1
    groups = lockstep_groups(sequences, bs) if track else [[[(0, p) for p in sequences[0][b0:b0 + bs]] for b0 in range(0, len(sequences[0]), bs)]]
    done, t0 = 0, time.perf_counter()
    wait = [0.0]

    def target(path, ext):
        d = os.path.join(out_dir, os.path.basename(os.path.dirname(os.path.abspath(path)))) if named else out_dir
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, os.path.splitext(os.path.basename(path))[0] + ext)

    def dump(path, rec):
        with open(path, 'w') as f:
            json.dump(rec, f)
    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), 16))) as dec, ThreadPoolExecutor(max_workers=8) as wr:
        jobs = []
        for steps in groups:
            ahead = {k: [dec.submit(decode_bgr, p) for _, p in steps[k]] for k in range(min(2, len(steps)))}

            def load(k):
                if k + 2 < len(steps):
                    ahead[k + 2] = [dec.submit(decode_bgr, p) for _, p in steps[k + 2]]
                w0 = time.perf_counter()
                frames = [f.result() for f in ahead.pop(k)]
                wait[0] += time.perf_counter() - w0
                return frames
            for st, recs, crops, outs in _walk(eng, steps, load, lambda e: e[1], lambda e, h, w: box_for(boxes, e[1], h, w), ratio, stage, track, False,
                                            antialias):
                if pictures:
                    over = V.overlay_predictions(outs[stage], crops, renderer)
                    if joints:
                        over = V.draw_joints(over, outs[stage]['pd_joint_uv_left'], outs[stage]['pd_joint_uv_right'])
                    ch, oh = crops.cpu().numpy(), over.cpu().numpy()
                if obj:
                    _, _, vl, vr = V.prediction_camera(outs[stage])
                    vh = np.concatenate([vl.cpu().numpy(), vr.cpu().numpy()], 1)
                for j, ((_, p), r) in enumerate(zip(st, recs)):
                    jobs.append(wr.submit(dump, target(p, '.json'), r))
                    if pictures:
                        jobs.append(wr.submit(write_png, target(p, '.png'), ch[j], oh[j]))
                    if obj:
                        jobs.append(wr.submit(write_obj, target(p, '.obj'), vh[j], faces))
                done += len(st)
        for j in jobs:
            j.result()
    return done, time.perf_counter() - t0, wait[0]


def main(argv=None):
    import argparse

    import torch

    from ..engine import DirEngine
    from ..utils import vis_utils as V
    from .dataset import gt_layers_from_checkpoint
    ap = argparse.ArgumentParser(description='run a DIR checkpoint on full-size photos or a video: GPU hand crops by box or by tracking, '
                                             'predictions in frame pixels')
    ap.add_argument('--model', type=str, required=True)
    ap.add_argument('--input', type=str, nargs='+', required=True, help='a directory of images, or image files')
    ap.add_argument('--out', type=str, required=True)
    ap.add_argument('--boxes', type=str, default=None, help='JSON {"name": [x0, y0, x1, y1]}: the tight box around both hands')
    ap.add_argument('--track', action='store_true', help='the input is a sequence (or one per sub-directory): every box after the first comes from the previous prediction')
    ap.add_argument('--ratio', type=float, default=0.8, help='the share of the crop the hands fill')
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--stage', type=int, default=2, choices=[0, 1, 2], help='0: the initial regression, 1 / 2: the refinement stages (2 = final)')
    ap.add_argument('--dtype', choices=['f16', 'bf16', 'f32'], default='f16')
    ap.add_argument('--workers', type=int, default=8, help='decode threads (at most 16)')
    ap.add_argument('--pictures', action='store_true', help='write <stem>.png: crop | overlay')
    ap.add_argument('--joints', action='store_true', help='draw the predicted 2-D joints on the overlay')
    ap.add_argument('--obj', action='store_true', help='write <stem>.obj: both predicted hands in one frame')
    ap.add_argument('--antialias', action='store_true', help='anti-aliased crops where the crop shrinks the frame (hand boxes larger than 256 px)')
    opt = ap.parse_args(argv)
    if opt.bs < 1:
        ap.error('--bs must be at least 1')
    sequences = list_sequences(opt.input) if opt.track else [list_images(opt.input)]
    if not any(sequences):
        raise ValueError('predict: no image files (%s) in %s' % (' / '.join(EXTENSIONS), opt.input))
    boxes = None
    if opt.boxes:
        with open(opt.boxes) as f:
            boxes = json.load(f)
    state = torch.load(opt.model, map_location='cpu', weights_only=False)
    state = state['net'] if isinstance(state, dict) and 'net' in state else state
    eng = DirEngine(state, dtype={'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[opt.dtype], root_joint=0)
    renderer = faces = None
    if opt.pictures or opt.obj:
        mano = gt_layers_from_checkpoint(state)
        faces = V.faces_from_layers(mano)
        if opt.pictures:
            renderer = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((V.NV_HAND, 3)), img_size=SIZE,
                                                        device=eng.device)
    n, sec, wait = run(eng, sequences, opt.out, boxes, opt.ratio, opt.stage, opt.bs, opt.track, opt.workers, opt.pictures, opt.joints, opt.obj,
                       renderer, faces, opt.antialias)
    print('waited %.2f s of them for decoded frames' % wait)
    print('%d images in %.1f s: %.0f images/s' % (n, sec, n / max(sec, 1e-9)))
    return n


if __name__ == '__main__':
    main()
