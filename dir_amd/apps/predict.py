"""The network on your own photos or a video: full-size frames of any size -> the crop the network was trained on (dir_amd.utils.crop, on
the GPU) -> DirEngine.forward -> predictions in FRAME pixels.

    python -m dir_amd.apps.predict --model CKPT --input DIR|FILES --out DIR [--boxes boxes.json] [--track] [--ratio 0.8] [--bs 32]
                                   [--stage 2] [--dtype f16|bf16|f32] [--workers 8] [--pictures] [--joints] [--obj] [--antialias]
                                   [--smooth] [--smooth_space point|para] [--shape_frames N] [--smooth_box] [--fps 30] [--min_cutoff 1.0] [--beta 0.007] [--d_cutoff 1.0]
                                   [--keypoints FILE] [--refine_iters 50] [--refine_lr 0.01] [--refine_prior 1e-3]

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

--smooth (with --track): every frame's prediction goes through the One-Euro filter (utils/smooth.py, csrc/smooth.hip: one launch per frame
over all streams of all sequences, state on the device, no host read) in FRAME space: meshes, 3-D joints and the offset in metres, 2-D
joints and cameras in frame pixels.  left / right / offset then hold the filtered values and "raw" what they are without the flag, bit for
bit: the crops and the forwards are the same.  --pictures, --joints and --obj draw the filtered prediction mapped back into the crop.  A
frame without a valid crop, or with a non-finite prediction, passes through unchanged (nulls stay nulls) and the filter takes the next
usable frame with dt = frames since the last one / --fps; after more than round(--fps) such frames it starts again.  --fps, --min_cutoff,
--beta, --d_cutoff are the filter's parameters; the defaults are the paper's (Casiez et al. 2012) and are NOT tuned on real video.  At the
end <out>/jitter.json (<out>/<sequence>/jitter.json with sub-directories) holds, per stream, the mean second difference per point per frame
of the raw and of the filtered values, and a line before the last one prints their means in mm/frame^2 and px/frame^2.
--smooth_space para (with --track --smooth; default point): the filter runs in MANO PARAMETER space instead (utils/smooth.py
ParameterSmoother, csrc/para_smooth.hip, the rule in include/dir_hip.h): the root rotation on SO(3), the 15 finger joints per joint in
axis-angle, the frame camera as three scalars, and ONE shape per sequence -- the betas are averaged over the first --shape_frames usable frames
(default round(--fps)) and then frozen.  left / right hold the mesh, joints and 2-D joints REGENERATED from the filtered parameters by the MANO
forward in the same launch (so the 2-D joints are the projection of the 3-D joints, which are the joints of the mesh, and bone lengths hold once
the shape is frozen); "mano" holds the parameters themselves and "shape_frozen" whether each hand's shape is fixed yet; jitter.json gains the
bone flicker (mean change of a bone's length from frame to frame, mm).  rot_speed_scale (100, a guess of 100 mm per radian) and the other
defaults are NOT tuned.  Without this flag every byte written is what it was.
--smooth_box (with --track, separate from --smooth, off by default): the next tracked box (its centre and half side) goes through a filter
of its own before the next crop is made, on the device; a first box and a held box are unchanged.  This changes the crops, and with them
every prediction after frame 1.  These flags without --track are an error.

--keypoints FILE: 2-D keypoints from an external detector or an annotator, a JSON object {"name": {"left": [[x, y, conf] x 21], "right": ...}}
keyed like --boxes; frame pixels, in the joint order of pd_joint_uv_*; a hand, or an image, may be absent, and a confidence of 0 drops a keypoint.
After the forward the stage's pd_mano_para_* are refined against them by dir_mano_fit (utils/mano_fit.py: --refine_iters Adam steps at
--refine_lr inside one launch, no host read): the keypoints go into crop coordinates (from_frame_pixels, rounded once), only the 2-D term and
the pull towards the network's own parameters (w_init = --refine_prior) are used, and the betas are frozen.  left / right then hold the fit's
meshes, joints, 2-D joints and cameras, "unrefined" what they are without the flag, bit for bit; a hand without a usable keypoint, or whose fit
reports a non-finite input or step, keeps the network's values ("refined_hands").  --track takes its next box from the refined meshes and
--smooth filters the refined values.  The defaults are NOT tuned on real keypoints; Adam's steps are lr-sized whatever the residual, so
keypoints the network already meets to a fraction of a pixel come back jittered at that scale.  Without --keypoints nothing changes.

--separate [--separate_iters 30 --separate_weight 1e4 --separate_prior 1e-2]: after the forward (and after the --keypoints refinement) the two hands of
every prediction go through the pair fit (dir_mano_fit_pair, utils/mano_fit.py fit_mano_pair) with three terms only: the pull to the prediction's own
parameters, the pull to its own offset (0.15 x pd_offset, the right root minus the left) and a capsule-per-bone collision term; the betas are frozen.
A prediction whose capsules overlap and whose fit reports nothing comes back pushed apart ("separated": true); every other one keeps its values bit
for bit.  Records gain "separated", "collision": {"before": {"mean_sq_overlap", "max_overlap"}, "after": {...}} (metres) and "unseparated" (left,
right, offset as they were).  --track and --smooth go on from the separated values.  The radii (capsule_radii of the checkpoint's tables) and the
weights are NOT tuned: this tree has no real MANO tables.  Without --separate nothing changes.

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
  smoothed, raw          only with --smooth: true, and {"left", "right", "offset"} as they are without the flag
  mano, shape_frozen     only with --smooth_space para: {"left": {"root_6d" [6], "pose_aa" [45] axis-angles with the mean included, "betas" [10],
                         "camera_px" [3]}, "right": ...} -- the filtered hand model behind left / right -- and [bool, bool]
  box_smoothed           only with --smooth_box: true where this frame's matrix went through the box filter
  refined, refined_hands, unrefined   only with --keypoints: true, {"left": bool, "right": bool} (which hands the fit replaced), and
                         {"left", "right"} as they are without the flag
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


def keypoints_for(kps, path):
    """the entry of --keypoints for a file (keys as box_for's: directory/name, directory/stem, name, stem), or None"""
    name = os.path.basename(path)
    stem, seq = os.path.splitext(name)[0], os.path.basename(os.path.dirname(os.path.abspath(path)))
    for k in (seq + '/' + name, seq + '/' + stem, name, stem):
        if kps and k in kps:
            return kps[k]
    return None


def keypoint_array(entries):
    """[{"left": [[x, y, conf] x 21], "right": ...} or None per image] -> float32 [B,2,21,3]; an absent hand or image: confidence 0"""
    out = np.zeros((len(entries), 2, 21, 3), np.float32)
    for i, e in enumerate(entries):
        for h, s in enumerate(SIDES):
            if e is not None and e.get(s) is not None:
                a = np.asarray(e[s], np.float32)
                if a.shape != (21, 3):
                    raise ValueError('predict: the keypoints of a hand must be [[x, y, conf] x 21], got shape %s' % (list(a.shape),))
                out[i, h] = a
    return out


class Tracker(object):
    """The crop of every frame of one or more sequences that advance in lockstep.

        tr = Tracker(eng, ratio=0.8, stage=2)
        crops, outs = tr.step(FrameBatch(frames_t), boxes_t0)     # boxes: [B,4] for the first step (None: whole frames), ignored afterwards

    A later step may bring fewer frames than the one before: the sequences at the tail of the batch have ended.  With track=False every
    step is a first step.

    After a step: `M` float64 [B,6] the matrices the crops were made with, `valid` int32 [B] whether a crop could be made, `tracked`
    int32 [B] whether the matrix came from the previous prediction (0 on the first step and where the box was held); all on the
    device.  The next matrices are made right after the forward, on the device, with no host read.  With antialias=True the crops are
    crop_frames(antialias=True) and `area` int32 [B] says which of them got the anti-aliased rule (None otherwise).

    smooth (True, or a dict of utils.smooth.OneEuro's parameters; needs track): after every forward the stage goes through a
    PredictionSmoother sized by the first step -- with 'space': 'para' in the dict (and optionally 'shape_frames', 'rot_speed_scale',
    'cam_speed_scale') through a ParameterSmoother on the stage's own MANO tables, the forward then run with want_para; `smoothed` is its result (frame space) and drawn(outs) the stage dict to draw.  smooth_box
    (likewise): the next matrices go through smooth_matrices before the next crop; `box_smoothed` int32 [B] says which of the current
    matrices did.  Neither reads anything back.

    refine (a dict with iters, lr, prior): step(..., keypoints=float32 [B,2,21,3] frame pixels | confidence) refines the stage's
    pd_mano_para_* against them with utils.mano_fit.fit_mano right after the forward, on the device: the stage dict of `outs` is then the
    refined one (tracking, smoothing and drawing go on from it), `unrefined` the network's own and `refined_hands` bool [B,2] which hands the
    fit replaced."""

    def __init__(self, eng, ratio=0.8, stage=2, size=SIZE, track=True, antialias=False, smooth=None, smooth_box=None, refine=None, separate=None):
        self.eng, self.ratio, self.stage, self.size, self.track = eng, float(ratio), int(stage), int(size), bool(track)
        self.antialias = bool(antialias)
        self.M = self.valid = self.tracked = self.area = None
        self._next = None
        self.smooth, self.smooth_box = (None if not p else ({} if p is True else dict(p)) for p in (smooth, smooth_box))
        if (self.smooth is not None or self.smooth_box is not None) and not self.track:
            raise ValueError('Tracker: smooth and smooth_box need track=True')
        self.smoother = self.box_filter = self.smoothed = self.box_smoothed = self._box_updated = None
        self.smooth_space = 'point' if self.smooth is None else self.smooth.pop('space', 'point')
        if self.smooth_space not in ('point', 'para'):
            raise ValueError("Tracker: smooth['space'] is 'point' or 'para', got %r" % (self.smooth_space,))
        if self.smooth_space == 'point' and 'shape_frames' in (self.smooth or {}):
            raise ValueError("Tracker: shape_frames needs smooth['space'] = 'para'")
        self.refine = None if refine is None else dict(refine)
        self.unrefined = self.refined_hands = None
        self.separate = None if separate is None else dict(separate)
        self.unseparated = self.separated = self.collision = None

    def _stage_tables(self):
        e = self.eng
        return e.init_mano if self.stage == 0 else (e.stage4, e.stage3)[self.stage - 1].mano if self.stage < 3 else e.stages_x[self.stage - 3].mano

    def _refine(self, o, keypoints):
        """the stage dict with the hands that have keypoints replaced by their fit (2-D term + prior, betas frozen)"""
        import torch

        from ..utils import crop as CR
        from ..utils import mano_fit as MF
        dev, B = self.eng.device, o['pd_mano_para_left'].shape[0]
        kp = torch.as_tensor(np.zeros((B, 2, 21, 3), np.float32) if keypoints is None else np.asarray(keypoints, np.float32).reshape(B, 2, 21, 3)).to(dev)
        uv, conf = [], []
        for h in range(2):
            c = kp[:, h, :, 2]
            c = torch.where(torch.isfinite(c) & (c > 0) & (self.valid[:, None] > 0), c, torch.zeros((), device=dev))
            u = CR.from_frame_pixels(kp[:, h, :, :2], self.M, self.size).float()              # rounded once
            uv.append(torch.where((c > 0)[..., None], u, torch.zeros((), device=dev)).contiguous())
            conf.append(c.contiguous())
        lr = float(self.refine.get('lr', 0.01))
        res = MF.fit_mano(list(self._stage_tables()), [o['pd_mano_para_left'], o['pd_mano_para_right']], joint_uv=uv, uv_conf=conf,
                          iters=int(self.refine.get('iters', 50)), lr={'root': lr, 'pca': lr, 'betas': 0.0, 'cam': lr},
                          weights={'w_uv': 1.0, 'w_init': float(self.refine.get('prior', 1e-3))})
        new, taken = dict(o), []
        for h, s in enumerate(SIDES):
            take = (conf[h] > 0).any(1) & ((res.status[h] & 6) == 0)
            taken.append(take)
            para = torch.where(take[:, None], res.para[h], o['pd_mano_para_' + s])
            new['pd_mano_para_' + s], new['pd_proj_' + s] = para, para[:, 61:64]
            for k, r in (('pd_mesh_xyz_', res.verts[h]), ('pd_joint_xyz_', res.joints[h]), ('pd_joint_uv_', res.joint_uv[h])):
                new[k + s] = torch.where(take[:, None, None], r.to(o[k + s].dtype), o[k + s])
        self.refined_hands = torch.stack(taken, 1)
        return new

    def _separate(self, o):
        """the stage dict with the pairs whose capsules overlap pushed apart by the pair fit: the pull to the prediction's own parameters (w_init) and to
        its own offset (w_off_init) against the collision term (w_col), betas frozen"""
        import torch

        from .. import _capi
        from ..utils import mano_fit as MF
        from ..utils.penetration import OFFSET_UNIT
        sp, B = self.separate, o['pd_mano_para_left'].shape[0]
        o0 = (OFFSET_UNIT * _capi.f32c(o['pd_offset']).reshape(B, 3)).contiguous()
        lr, w_col = float(sp.get('lr', 0.005)), float(sp.get('weight', 1e4))
        res = MF.fit_mano_pair(list(self._stage_tables()), [o['pd_mano_para_left'], o['pd_mano_para_right']], o0, radii=sp['radii'], iters=int(sp.get('iters', 30)),
                               lr={'root': lr, 'pca': lr, 'betas': 0.0, 'cam': lr, 'offset': lr},
                               weights={'w_init': float(sp.get('prior', 1e-2)), 'w_off_init': float(sp.get('offset_prior', 1.0)), 'w_col': w_col})
        take = (res.pair_status == 0) & ((res.status[0] & 6) == 0) & ((res.status[1] & 6) == 0) & (res.collision[:, 1] > 0) & (self.valid > 0)
        if not w_col > 0:
            take = torch.zeros_like(take)                                  # nothing pushes: every pair keeps the network's values
        new = dict(o)
        for h, s in enumerate(SIDES):
            para = torch.where(take[:, None], res.para[h], o['pd_mano_para_' + s])
            new['pd_mano_para_' + s], new['pd_proj_' + s] = para, para[:, 61:64]
            for k, r in (('pd_mesh_xyz_', res.verts[h]), ('pd_joint_xyz_', res.joints[h]), ('pd_joint_uv_', res.joint_uv[h])):
                new[k + s] = torch.where(take[:, None, None], r.to(o[k + s].dtype), o[k + s])
        off = (res.offset / OFFSET_UNIT).reshape(o['pd_offset'].shape).to(o['pd_offset'].dtype)
        new['pd_offset'] = torch.where(take.reshape([B] + [1] * (off.dim() - 1)), off, o['pd_offset'])
        self.separated = take
        self.collision = torch.where(take[:, None], res.collision, torch.cat([res.collision[:, :2], res.collision[:, :2]], 1))
        return new

    def drawn(self, outs):
        """the stage dict to draw: the smoothed prediction in the current crop, or the stage itself"""
        return self.smoother.crop_stage() if self.smoother is not None else outs[self.stage]

    def step(self, batch, boxes=None, keypoints=None):
        import torch

        from ..utils import crop as CR
        dev, B = self.eng.device, len(batch)
        if self._next is None or not self.track:
            if boxes is None:
                boxes = [[0.0, 0.0, w - 1.0, h - 1.0] for h, w in batch.sizes]
            b = torch.as_tensor(np.asarray(boxes, np.float32).reshape(B, 4)).to(dev)
            self.M, self.valid = CR.crop_matrices_from_boxes(b, self.ratio, self.size)
            self.tracked = torch.zeros(B, dtype=torch.int32, device=dev)
            if self.smooth_box is not None:
                self.box_smoothed = torch.zeros(B, dtype=torch.int32, device=dev)
        else:
            if self._next[0].shape[0] < B:
                raise ValueError('Tracker.step: %d frames after %d: sequences may end (from the tail of the batch), not begin' % (B, self._next[0].shape[0]))
            M, ok, prev_valid = (x[:B].contiguous() for x in self._next)
            # a held box is as good as it was: the crop stays valid where the previous one was
            self.M, self.tracked, self.valid = M, ok, torch.maximum(ok, prev_valid)
            if self.smooth_box is not None:
                self.box_smoothed = (self._box_updated[:B] == 1).to(torch.int32)
        if self.antialias:
            crops, status, self.area = CR.crop_frames(batch, self.M, self.valid, self.size, return_status=True, antialias=True, return_area=True)
        else:
            crops, status = CR.crop_frames(batch, self.M, self.valid, self.size, return_status=True)
        self.valid = self.valid * (status == 0).to(torch.int32)            # a crop the kernel refused is black: the image is not valid
        if self.refine is None and self.separate is None and self.smooth_space == 'para':
            outs = self.eng.forward(crops, want_proj_feat=False, want_para=True)
        elif self.refine is None and self.separate is None:
            outs = self.eng.forward(crops, want_proj_feat=False)
        else:
            outs = list(self.eng.forward(crops, want_proj_feat=False, want_para=True))
            if self.refine is not None:
                self.unrefined = outs[self.stage]
                outs[self.stage] = self._refine(outs[self.stage], keypoints)
            if self.separate is not None:
                self.unseparated = outs[self.stage]
                outs[self.stage] = self._separate(outs[self.stage])
        if self.track:
            M_next, ok = CR.crop_matrices_from_meshes(outs[self.stage], self.M, self.ratio, self.size)
            if self.smooth_box is not None:
                from ..utils import smooth as SM
                if self.box_filter is None:
                    self.box_filter = SM.box_filter(B, device=dev, **self.smooth_box)
                M_next, self._box_updated = SM.smooth_matrices(self.box_filter, M_next, ok, self.size)
            self._next = (M_next, ok, self.valid)
        if self.smooth is not None:
            from ..utils import smooth as SM
            if self.smoother is None and self.smooth_space == 'para':
                self.smoother = SM.ParameterSmoother(list(self._stage_tables()), B, self.size, device=dev, **self.smooth)
            elif self.smoother is None:
                self.smoother = SM.PredictionSmoother(B, self.size, device=dev, **self.smooth)
            self.smoothed = self.smoother.step(outs[self.stage], self.M, self.valid)
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
    un = tr.unrefined if tr.refine is not None else None
    if un is not None:
        t['refined_hands'] = tr.refined_hands
        for s in SIDES:
            t['u_px_' + s] = CR.to_frame_pixels(un['pd_joint_uv_' + s].float(), M, tr.size)
            t['u_xyz_' + s] = un['pd_joint_xyz_' + s].float()
            t['u_sc_' + s], t['u_tr_' + s] = CR.frame_camera(un['pd_proj_' + s].float(), M, tr.size)
        if keep_stage:
            for k in ('pd_mesh_xyz_left', 'pd_mesh_xyz_right', 'pd_proj_left', 'pd_proj_right', 'pd_joint_uv_left', 'pd_joint_uv_right'):
                t['u_' + k] = un[k].float()
    us = tr.unseparated if tr.separate is not None else None
    if us is not None:
        t['separated'], t['collision'], t['p_offset'] = tr.separated, tr.collision, us['pd_offset'].float()
        for s in SIDES:
            t['p_px_' + s] = CR.to_frame_pixels(us['pd_joint_uv_' + s].float(), M, tr.size)
            t['p_xyz_' + s] = us['pd_joint_xyz_' + s].float()
            t['p_sc_' + s], t['p_tr_' + s] = CR.frame_camera(us['pd_proj_' + s].float(), M, tr.size)
    fr = tr.smoothed if tr.smooth is not None else None
    if fr is not None:
        t['s_offset'] = fr['offset']
        for s in SIDES:
            t['s_px_' + s], t['s_xyz_' + s], t['s_cam_' + s] = fr['joints_px_' + s], fr['joint_xyz_' + s], fr['camera_px_' + s]
            if tr.smooth_space == 'para':
                t['s_mano_' + s] = fr['smoothed_' + s]
        if tr.smooth_space == 'para':
            t['s_shape_count'] = fr['shape_count']
        if keep_stage:
            t.update(('s_' + k, v) for k, v in tr.smoother.crop_stage().items())
    if tr.box_smoothed is not None:
        t['box_smoothed'] = tr.box_smoothed
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
        if un is not None:
            r['unrefined'] = {s: {'joints_px': num(h['u_px_' + s][j].tolist()), 'joints_xyz': num(h['u_xyz_' + s][j].tolist()),
                                  'camera_px': {'scale': num(float(h['u_sc_' + s][j])), 'trans': num(h['u_tr_' + s][j].tolist())}} for s in SIDES}
            r['refined'] = True
            r['refined_hands'] = {s: bool(h['refined_hands'][j][i]) for i, s in enumerate(SIDES)}
        if us is not None:
            r['unseparated'] = {s: {'joints_px': num(h['p_px_' + s][j].tolist()), 'joints_xyz': num(h['p_xyz_' + s][j].tolist()),
                                    'camera_px': {'scale': num(float(h['p_sc_' + s][j])), 'trans': num(h['p_tr_' + s][j].tolist())}} for s in SIDES}
            r['unseparated']['offset'] = num(h['p_offset'][j].reshape(-1).tolist())
            r['separated'] = bool(h['separated'][j])
            c = [float(x) for x in h['collision'][j]]
            r['collision'] = {'before': {'mean_sq_overlap': num(c[0]), 'max_overlap': num(c[1])}, 'after': {'mean_sq_overlap': num(c[2]), 'max_overlap': num(c[3])}}
        if fr is not None:                                                # the fields above are today's: they move to "raw"
            r['raw'] = {k: r[k] for k in SIDES + ('offset',)}
            for s in SIDES:
                r[s] = {'joints_px': num(h['s_px_' + s][j].tolist()), 'joints_xyz': num(h['s_xyz_' + s][j].tolist()),
                        'camera_px': {'scale': num(float(h['s_cam_' + s][j][0])), 'trans': num(h['s_cam_' + s][j][1:3].tolist())}}
            r['offset'] = num(h['s_offset'][j].reshape(-1).tolist())
            r['smoothed'] = True
            if 's_shape_count' in h:                                          # smooth_space para: the hand model behind left / right
                r['mano'] = {s: {'root_6d': num(h['s_mano_' + s][j][0:6].tolist()), 'pose_aa': num(h['s_mano_' + s][j][6:51].tolist()),
                                 'betas': num(h['s_mano_' + s][j][51:61].tolist()), 'camera_px': num(h['s_mano_' + s][j][61:64].tolist())} for s in SIDES}
                n = tr.smoother.shape_frames
                r['shape_frozen'] = [bool(n > 0 and c >= n) for c in h['s_shape_count'][j].tolist()]
        if 'box_smoothed' in h:
            r['box_smoothed'] = bool(h['box_smoothed'][j])
        if 'area' in h:
            r['antialiased'] = bool(h['area'][j])
        if keep_stage:
            r['stage'] = {k: h[k][j] for k in h if k.startswith('pd_')}
            if un is not None:
                r['stage_unrefined'] = {k[2:]: h[k][j] for k in h if k.startswith('u_pd_')}
            if fr is not None:
                r['stage_smoothed'] = {k[2:]: h[k][j] for k in h if k.startswith('s_pd_')}
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


def _walk(eng, steps, load, names, box_of, ratio, stage, track, keep_stage, antialias=False, smooth=None, smooth_box=None, refine=None, kp_of=None, separate=None):
    """the one loop: per step FrameBatch -> Tracker.step -> records.  load(k) -> the decoded frames of step k; box_of(entry, h, w) -> the
    box of a step entry; kp_of(step index, entry) -> its keypoints entry or None (with refine).  Yields (entries, records, crops, outs, tracker)
    with the device tensors of that step."""
    from ..utils import crop as CR
    tr = Tracker(eng, ratio, stage, track=track, antialias=antialias, smooth=smooth, smooth_box=smooth_box, refine=refine, separate=separate)
    for k, st in enumerate(steps):
        batch = CR.FrameBatch(load(k))
        used = [box_of(e, h, w) for e, (h, w) in zip(st, batch.sizes)] if (not track or k == 0) else None
        if refine is not None:
            crops, outs = tr.step(batch, used, keypoint_array([kp_of(k, e) for e in st]))
        else:
            crops, outs = tr.step(batch, used)
        yield st, _records([names(e) for e in st], batch, used, tr, outs, stage, keep_stage), crops, outs, tr


def sequence_jitter(tr, steps):
    """after a walk with smooth: one host read -> {sequence index: the jitter of its row as JSON fields}.  Per stream (PredictionSmoother's
    order) the mean |second difference| per point per frame of the raw and of the filtered values -- metres for mesh_xyz, joint_xyz and offset, frame
    pixels for joints_px; camera_px mixes pixels per metre and pixels -- over `frames` frames (every third and later of consecutive updates)"""
    from ..utils import smooth as SM
    j = tr.smoother.jitter()

    def num(a):
        return [v if np.isfinite(v) else None for v in a.tolist()]
    out = {i: {'streams': j['streams'], 'points': [p for _, p, _, _ in SM.STREAMS], 'frames': int(j['frames'][row]), 'raw': num(j['raw'][row]),
               'filtered': num(j['filtered'][row]), 'sums': j['sums'][row].tolist()} for row, (i, _) in enumerate(steps[0])}
    if 'bone_flicker' in j:                        # smooth_space para: a hand counts its own frames; bone flicker in mm per bone per frame
        f = j['bone_flicker']
        for row, (i, _) in enumerate(steps[0]):
            out[i].update(space='para', stream_frames=j['stream_frames'][row].tolist(),
                          bone_flicker={'hands': list(SIDES), 'bones': 20, 'frames': f['frames'][row].tolist(), 'raw_mm': num(f['raw'][row] * 1000.0),
                                        'filtered_mm': num(f['filtered'][row] * 1000.0), 'sums': f['sums'][row].tolist()})
    return out


def jitter_summary(jitters):
    """[sequence_jitter records] -> ((raw, filtered) in mm/frame^2 over the metric streams, (raw, filtered) in px/frame^2 over joints_px),
    means per point per frame over all sequences; NaN when no frame was counted"""
    mm, px = np.zeros(3), np.zeros(3)
    for j in jitters:
        frames = j.get('stream_frames', [j['frames']] * len(j['streams']))
        for name, p, (raw, fil), n in zip(j['streams'], j['points'], j['sums'], frames):
            if name.startswith('camera_px'):
                continue
            acc = px if name.startswith('joints_px') else mm
            acc += (raw, fil, p * n)
    with np.errstate(invalid='ignore', divide='ignore'):
        return tuple(mm[:2] / mm[2] * 1000.0), tuple(px[:2] / px[2])


def flicker_summary(jitters):
    """[sequence_jitter records of a smooth_space para walk] -> (raw, filtered) bone flicker in mm per bone per frame over all sequences and hands"""
    acc = np.zeros(3)
    for j in jitters:
        f = j['bone_flicker']
        for (raw, fil), n in zip(f['sums'], f['frames']):
            acc += (raw, fil, f['bones'] * n)
    with np.errstate(invalid='ignore', divide='ignore'):
        return tuple(acc[:2] / acc[2] * 1000.0)


def predict(eng, frames, boxes=None, ratio=0.8, stage=2, bs=32, track=False, keep_stage=False, keep_crops=False, antialias=False, smooth=None,
            smooth_box=None, return_jitter=False, keypoints=None, refine_iters=50, refine_lr=0.01, refine_prior=1e-3, separate=None):
    """The loop behind the command, on decoded frames.

    frames: without `track` a list of uint8 BGR arrays [H,W,3] of any sizes, taken `bs` at a time; with `track` a list of sequences (each
    a list of frames), advanced in lockstep -- one frame of every sequence per forward, a shorter sequence dropping out at its end; more
    than `bs` sequences walk `bs` at a time, one group after the other.
    boxes: one (x0, y0, x1, y1) or None per image (with `track` per sequence: the box of its frame 0); None: whole frames.
    -> a list of records (the JSON fields; with `track` one list per sequence), each with 'crop' (uint8 [256,256,3]) when keep_crops and
    'stage' (the stage's meshes, projections and joint uv as numpy arrays) when keep_stage.  antialias: anti-aliased crops where a crop
    shrinks its frame; every record then has 'antialiased'.
    smooth / smooth_box (with `track`; True or a dict of utils.smooth.OneEuro's parameters): Tracker's.  With smooth a record's left, right
    and offset are filtered, 'raw' holds the unfiltered ones, and keep_stage adds 'stage_smoothed' (PredictionSmoother.crop_stage);
    smooth={'space': 'para', ...} smooths in MANO parameter space instead (utils.smooth.ParameterSmoother: records gain 'mano' and 'shape_frozen', the
    jitter records 'bone_flicker');
    return_jitter -> (records, [sequence_jitter per sequence]).
    keypoints: one {"left": [[x, y, conf] x 21], "right": ...} or None per image (with `track` one such list per sequence), frame pixels: the
    stage is refined against them (the module docstring's --keypoints; refine_iters, refine_lr, refine_prior); every record then has
    'unrefined', 'refined' and 'refined_hands', and keep_stage adds 'stage_unrefined'.  None: nothing changes.
    separate: a dict with 'radii' (two [20] GPU tensors, utils.mano_fit.capsule_radii) and optionally iters, weight, prior, offset_prior, lr: after the
    forward (and the refinement) every prediction goes through the pair fit (the module docstring's --separate); every record then has 'separated',
    'collision' and 'unseparated'.  None: nothing changes."""
    refine = None if keypoints is None else {'iters': refine_iters, 'lr': refine_lr, 'prior': refine_prior}

    def kp_of(k, e):
        entry = keypoints[e[0]]
        return (entry[k] if k < len(entry) else None) if track and entry is not None else entry
    if (smooth or smooth_box) and not track:
        raise ValueError('predict: smooth and smooth_box need track=True')
    if return_jitter and not smooth:
        raise ValueError('predict: return_jitter needs smooth')
    jit = [None] * len(frames)
    if track:
        groups = lockstep_groups([list(s) for s in frames], bs)
        out = [[] for _ in frames]
    else:
        groups = [[[(i, frames[i]) for i in range(b0, min(b0 + bs, len(frames)))] for b0 in range(0, len(frames), bs)]]
        out = [None] * len(frames)

    def box_of(e, h, w):
        return [float(v) for v in boxes[e[0]]] if boxes is not None and boxes[e[0]] is not None else [0.0, 0.0, w - 1.0, h - 1.0]
    for steps in groups:
        tr = None
        for st, recs, crops, outs, tr in _walk(eng, steps, lambda k: [f for _, f in steps[k]], lambda e: str(e[0]), box_of, ratio, stage, track,
                                                keep_stage, antialias, smooth, smooth_box, refine, kp_of, separate):
            ch = crops.cpu().numpy() if keep_crops else None
            for j, ((i, _), r) in enumerate(zip(st, recs)):
                if keep_crops:
                    r['crop'] = ch[j]
                if track:
                    out[i].append(r)
                else:
                    out[i] = r
        if return_jitter and tr is not None:
            for i, j in sequence_jitter(tr, steps).items():
                jit[i] = j
    return (out, jit) if return_jitter else out


def run(eng, sequences, out_dir, boxes=None, ratio=0.8, stage=2, bs=32, track=False, workers=8, pictures=False, joints=False, obj=False,
        renderer=None, faces=None, antialias=False, smooth=None, smooth_box=None, jitter_out=None, keypoints=None, refine=None, separate=None):
    """files -> files.  sequences: [[paths]] (one list without `track`).  -> (images, seconds, seconds of them spent waiting for decoded
    frames).  Two steps are decoded ahead of the GPU by at most 16 threads; the files are written by 8 more.  With `track`, more than `bs`
    sequences walk `bs` at a time, so that no batch holds more than `bs` images.  smooth / smooth_box: Tracker's; with smooth the pictures
    and OBJs show the filtered prediction, every sequence gets a jitter.json, and a list given as jitter_out receives their contents.
    keypoints: the --keypoints object (keypoints_for's keys) with refine = {'iters', 'lr', 'prior'}: every stage is refined against them.
    separate: predict()'s."""
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
            tr = None
            for st, recs, crops, outs, tr in _walk(eng, steps, load, lambda e: e[1], lambda e, h, w: box_for(boxes, e[1], h, w), ratio, stage, track,
                                                    False, antialias, smooth, smooth_box, (refine or {}) if keypoints is not None else None,
                                                    lambda k, e: keypoints_for(keypoints, e[1]), separate):
                shown = tr.drawn(outs) if pictures or obj else None
                if pictures:
                    over = V.overlay_predictions(shown, crops, renderer)
                    if joints:
                        over = V.draw_joints(over, shown['pd_joint_uv_left'], shown['pd_joint_uv_right'])
                    ch, oh = crops.cpu().numpy(), over.cpu().numpy()
                if obj:
                    _, _, vl, vr = V.prediction_camera(shown)
                    vh = np.concatenate([vl.cpu().numpy(), vr.cpu().numpy()], 1)
                for j, ((_, p), r) in enumerate(zip(st, recs)):
                    jobs.append(wr.submit(dump, target(p, '.json'), r))
                    if pictures:
                        jobs.append(wr.submit(write_png, target(p, '.png'), ch[j], oh[j]))
                    if obj:
                        jobs.append(wr.submit(write_obj, target(p, '.obj'), vh[j], faces))
                done += len(st)
            if smooth and tr is not None:
                for i, j in sequence_jitter(tr, steps).items():
                    jobs.append(wr.submit(dump, os.path.join(os.path.dirname(target(sequences[i][0], '.json')), 'jitter.json'), j))
                    if jitter_out is not None:
                        jitter_out.append(j)
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
    ap.add_argument('--ema', action='store_true', help="load the averaged weights (the checkpoint's 'ema' key, written by dir_amd.apps.train --ema_decay) instead of 'net'")
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
    ap.add_argument('--smooth', action='store_true', help='with --track: One-Euro temporal smoothing of every prediction stream, in frame space; writes jitter.json')
    ap.add_argument('--smooth_space', choices=['point', 'para'], default='point',
                    help='with --track --smooth: filter every output point on its own (point), or the MANO parameters -- root rotation on SO(3), finger joints in '
                         'axis-angle, one shape per sequence -- and regenerate mesh and joints from them (para)')
    ap.add_argument('--shape_frames', type=int, default=None, help='with --smooth_space para: the usable frames the shape is averaged over before it is frozen '
                                                                   '(default round(fps); 0: the betas pass through)')
    ap.add_argument('--smooth_box', action='store_true', help='with --track: smooth the next tracked box before the next crop is made (changes the crops)')
    ap.add_argument('--fps', type=float, default=None, help='the frame rate of the sequence (default 30)')
    ap.add_argument('--min_cutoff', type=float, default=None, help='One-Euro: the cutoff at rest, Hz (default 1.0, the paper\'s; not tuned on real video)')
    ap.add_argument('--beta', type=float, default=None, help='One-Euro: cutoff per speed, Hz per (mm/s or px/s) (default 0.007)')
    ap.add_argument('--d_cutoff', type=float, default=None, help='One-Euro: the cutoff of the speed estimate, Hz (default 1.0)')
    ap.add_argument('--keypoints', type=str, default=None, help='JSON {"name": {"left": [[x, y, conf] x 21], "right": ...}}: 2-D keypoints in frame pixels the prediction is refined against')
    ap.add_argument('--refine_iters', type=int, default=None, help='with --keypoints: Adam steps of the refinement (default 50; not tuned on real keypoints)')
    ap.add_argument('--refine_lr', type=float, default=None, help='with --keypoints: their learning rate (default 0.01)')
    ap.add_argument('--refine_prior', type=float, default=None, help="with --keypoints: the weight of the pull towards the network's own parameters (default 1e-3)")
    ap.add_argument('--separate', action='store_true', help='push interpenetrating hands apart: the pair fit with a capsule-per-bone collision term after the forward')
    ap.add_argument('--separate_iters', type=int, default=None, help='with --separate: Adam steps (default 30; not tuned)')
    ap.add_argument('--separate_weight', type=float, default=None, help='with --separate: the weight of the collision term (default 1e4; 0: nothing moves)')
    ap.add_argument('--separate_prior', type=float, default=None, help="with --separate: the weight of the pull towards the prediction's own parameters (default 1e-2)")
    opt = ap.parse_args(argv)
    if opt.bs < 1:
        ap.error('--bs must be at least 1')
    sp = {k: getattr(opt, 'separate_' + k) for k in ('iters', 'weight', 'prior') if getattr(opt, 'separate_' + k) is not None}
    if sp and not opt.separate:
        ap.error('--separate_iters, --separate_weight and --separate_prior need --separate')
    if min(sp.values(), default=0) < 0:
        ap.error('--separate_iters, --separate_weight and --separate_prior must not be negative')
    params = {k: getattr(opt, k) for k in ('fps', 'min_cutoff', 'beta', 'd_cutoff') if getattr(opt, k) is not None}
    if (opt.smooth or opt.smooth_box or params) and not opt.track:
        ap.error('--smooth, --smooth_box, --fps, --min_cutoff, --beta and --d_cutoff need --track')
    if params and not (opt.smooth or opt.smooth_box):
        ap.error('--fps, --min_cutoff, --beta and --d_cutoff need --smooth or --smooth_box')
    if any(v <= 0 for k, v in params.items() if k != 'beta') or params.get('beta', 0.0) < 0:
        ap.error('--fps, --min_cutoff and --d_cutoff must be positive and --beta not negative')
    if (opt.smooth_space != 'point' or opt.shape_frames is not None) and not (opt.track and opt.smooth):
        ap.error('--smooth_space and --shape_frames need --track --smooth')
    if opt.shape_frames is not None and (opt.smooth_space != 'para' or opt.shape_frames < 0):
        ap.error('--shape_frames needs --smooth_space para and must not be negative')
    rp = {k: getattr(opt, 'refine_' + k) for k in ('iters', 'lr', 'prior') if getattr(opt, 'refine_' + k) is not None}
    if rp and not opt.keypoints:
        ap.error('--refine_iters, --refine_lr and --refine_prior need --keypoints')
    if rp.get('iters', 1) < 0 or rp.get('lr', 1.0) < 0 or rp.get('prior', 1.0) < 0:
        ap.error('--refine_iters, --refine_lr and --refine_prior must not be negative')
    sequences = list_sequences(opt.input) if opt.track else [list_images(opt.input)]
    if not any(sequences):
        raise ValueError('predict: no image files (%s) in %s' % (' / '.join(EXTENSIONS), opt.input))
    boxes = None
    if opt.boxes:
        with open(opt.boxes) as f:
            boxes = json.load(f)
    keypoints = None
    if opt.keypoints:
        with open(opt.keypoints) as f:
            keypoints = json.load(f)
    state = torch.load(opt.model, map_location='cpu', weights_only=False)
    from . import checkpoint_weights
    state = checkpoint_weights(state, opt.ema, opt.model)
    eng = DirEngine(state, dtype={'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[opt.dtype], root_joint=0)
    renderer = faces = None
    if opt.pictures or opt.obj:
        mano = gt_layers_from_checkpoint(state)
        faces = V.faces_from_layers(mano)
        if opt.pictures:
            renderer = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((V.NV_HAND, 3)), img_size=SIZE,
                                                        device=eng.device)
    separate = None
    if opt.separate:
        from ..utils import mano_fit as MF
        from .fit_mano import layer_buffers
        separate = dict(sp, radii=[MF.capsule_radii(layer_buffers(state, s)).to(eng.device) for s in SIDES])
    jitters = []
    smooth_arg = (params or True) if opt.smooth else None
    if opt.smooth and opt.smooth_space == 'para':
        smooth_arg = dict(params, space='para', **({} if opt.shape_frames is None else {'shape_frames': opt.shape_frames}))
    n, sec, wait = run(eng, sequences, opt.out, boxes, opt.ratio, opt.stage, opt.bs, opt.track, opt.workers, opt.pictures, opt.joints, opt.obj,
                       renderer, faces, opt.antialias, smooth_arg, (params or True) if opt.smooth_box else None, jitters, keypoints, rp, separate)
    print('waited %.2f s of them for decoded frames' % wait)
    if opt.smooth:
        mm, px = jitter_summary(jitters)
        print('jitter, raw -> smoothed: %.4g -> %.4g mm/frame^2 (meshes, 3-D joints, offset), %.4g -> %.4g px/frame^2 (2-D joints)' % (mm + px))
        if opt.smooth_space == 'para':
            print('bone flicker, raw -> smoothed: %.4g -> %.4g mm/frame per bone' % flicker_summary(jitters))
    print('%d images in %.1f s: %.0f images/s' % (n, sec, n / max(sec, 1e-9)))
    return n


if __name__ == '__main__':
    main()
