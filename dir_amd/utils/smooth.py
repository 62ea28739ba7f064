"""Temporal smoothing of tracked predictions on the GPU: csrc/smooth.hip through dir_one_euro_step.  The One-Euro filter (Casiez, Roussel,
Vogel, CHI 2012) is an exponential filter whose cutoff rises with the filtered speed: it smooths a resting hand and follows a fast one.
The reference has no temporal code; the rule is written out in include/dir_hip.h and restated in float64 numpy by
tests/helpers/one_euro_ref.py.  One launch per frame over every stream of every sequence, state updated in place, no host read.

  OneEuro              the filter over rows of segments (n_points, dims, speed_scale); step(), jitter(), reset()
  PredictionSmoother   one stage of DirEngine.forward + the crop matrices -> frame-space streams -> one OneEuro step; crop_stage() maps the
                       smoothed values back into the crop as a stage dict that overlay_predictions / draw_joints / prediction_camera take
  smooth_matrices      the next tracked box (crop_matrices_from_meshes' M_next) through a OneEuro of its own

The defaults (min_cutoff 1 Hz, beta 0.007, d_cutoff 1 Hz) are the paper's; they are NOT tuned on real video.
"""
import ctypes

import numpy as np
import torch

from .. import _capi
from . import crop as CR

MAX_SEGMENTS, MAX_VALUES = 16, 16384                    # DIR_ONE_EURO_MAX_SEGMENTS, DIR_ONE_EURO_MAX_VALUES
PASSED, UPDATED, INITIALISED = 0, 1, 2                  # `updated`
_FIELDS = ('jitter', 'y1', 'y2', 'x1', 'x2', 'dxhat', 'age', 'run', 'count')
SIDES = ('left', 'right')


class OneEuro(object):
    """dir_one_euro_step over `batch` sequences.  segments: [(n_points, dims 1..4, speed_scale)], at most 16, sum n_points * dims <= 16384;
    a point gets one cutoff, fc = min_cutoff + beta * speed_scale * |dxhat|.  max_gap (frames, default round(fps)): a sequence whose last
    update is older starts again.

        y, updated = f.step(x, valid=None)      x float32 cuda [B,F], B <= batch (sequences end from the tail); valid int32 [B] or None
                                                updated int32 [B]: 0 passed through (not valid, or a non-finite input: y = x bit for bit),
                                                1 filtered, 2 initialised (y = x).  out=x filters in place.
        f.jitter()                              one host read -> {'raw', 'filtered': float64 [batch,S] mean |second difference| per point
                                                per frame (NaN before a third consecutive update), 'frames': int [batch], 'sums': [batch,S,2]}
        f.reset(rows=None)                      forget everything (or the listed rows)"""

    def __init__(self, segments, batch, fps=30.0, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, max_gap=None, device='cuda'):
        self.segments = [(int(n), int(d), float(s)) for n, d, s in segments]
        self.F, self.S, self.batch = sum(n * d for n, d, _ in self.segments), len(self.segments), int(batch)
        self.fps, self.min_cutoff, self.beta, self.d_cutoff = float(fps), float(min_cutoff), float(beta), float(d_cutoff)
        self.max_gap = int(round(self.fps)) if max_gap is None else int(max_gap)
        if not 1 <= self.S <= MAX_SEGMENTS or any(not 1 <= d <= 4 or n < 1 for n, d, _ in self.segments) or not 1 <= self.F <= MAX_VALUES:
            raise ValueError('OneEuro: need 1..%d segments (n_points >= 1, dims 1..4, speed_scale) of at most %d values together, got %r'
                             % (MAX_SEGMENTS, MAX_VALUES, segments))
        if not 1 <= self.batch <= CR.MAX_BATCH:
            raise ValueError('OneEuro: the batch must hold 1..%d sequences, got %d' % (CR.MAX_BATCH, self.batch))
        if not (self.fps > 0 and self.min_cutoff > 0 and self.d_cutoff > 0 and self.beta >= 0 and self.max_gap >= 1):
            raise ValueError('OneEuro: fps, min_cutoff and d_cutoff must be > 0, beta >= 0 and max_gap >= 1')
        self._segs = (_capi.OneEuroSegment * self.S)(*[_capi.OneEuroSegment(n, d, s) for n, d, s in self.segments])
        off = (ctypes.c_longlong * 9)()
        self.row_bytes = int(_capi.lib().dir_one_euro_state_bytes(self.F, self.S, off))
        if self.row_bytes < 0:
            raise ValueError('OneEuro: dir_one_euro_state_bytes refused F = %d, S = %d' % (self.F, self.S))
        self.offsets = dict(zip(_FIELDS, (int(v) for v in off)))
        self.device = torch.device(device)
        self.state = torch.zeros(self.batch, self.row_bytes, dtype=torch.uint8, device=self.device)

    def field(self, name):
        """a view of the state: 'y1' / 'y2' / 'x1' / 'x2' / 'dxhat' float32 [batch,F], 'age' / 'run' / 'count' int32 [batch,1], 'jitter'
        float64 [batch,S,2]"""
        o = self.offsets[name]
        if name == 'jitter':
            return self.state[:, o:o + 16 * self.S].view(torch.float64).view(self.batch, self.S, 2)
        if name in ('age', 'run', 'count'):
            return self.state[:, o:o + 4].view(torch.int32)
        return self.state[:, o:o + 4 * self.F].view(torch.float32)

    def step(self, x, valid=None, out=None):
        _capi.require_cuda(x, valid, out)
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.F or not x.is_contiguous() or x.device != self.state.device:
            raise ValueError('OneEuro.step: x must be a contiguous float32 [B,%d] tensor on %s, got %s %s' % (self.F, self.state.device, x.dtype, tuple(x.shape)))
        B = x.shape[0]
        if not 1 <= B <= self.batch:
            raise ValueError('OneEuro.step: %d rows for a state of %d: sequences may end (from the tail of the batch), not begin' % (B, self.batch))
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (B,) or not valid.is_contiguous() or valid.device != x.device):
            raise ValueError('OneEuro.step: valid must be a contiguous int32 [%d] tensor on %s' % (B, x.device))
        y = torch.empty_like(x) if out is None else out
        if y.dtype != torch.float32 or y.shape != x.shape or not y.is_contiguous() or y.device != x.device:
            raise ValueError('OneEuro.step: out must be like x')
        updated = torch.empty(B, dtype=torch.int32, device=x.device)
        P = _capi.ptr
        with torch.cuda.device(x.device):
            _capi.check(_capi.lib().dir_one_euro_step(P(x), P(valid), B, self._segs, self.S, self.fps, self.min_cutoff, self.beta, self.d_cutoff,
                                                      self.max_gap, P(self.state), P(y), P(updated), _capi.stream_ptr()), 'dir_one_euro_step')
        return y, updated

    def jitter(self):
        o = self.offsets
        h = torch.cat((self.state[:, o['jitter']:o['jitter'] + 16 * self.S], self.state[:, o['count']:o['count'] + 4]), 1).cpu().numpy()
        sums = np.ascontiguousarray(h[:, :16 * self.S]).view(np.float64).reshape(self.batch, self.S, 2)
        frames = np.ascontiguousarray(h[:, 16 * self.S:]).view(np.int32).reshape(self.batch).astype(np.int64)
        n = np.array([s[0] for s in self.segments], np.float64)[None, :, None]
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = sums / n / frames[:, None, None].astype(np.float64)
        return {'raw': mean[:, :, 0], 'filtered': mean[:, :, 1], 'frames': frames, 'sums': sums}

    def reset(self, rows=None):
        if rows is None:
            self.state.zero_()
        else:
            self.state[torch.as_tensor(list(rows), dtype=torch.long, device=self.state.device)] = 0


# the streams of one hand, in the order they are packed: name, points, dims, speed scale.  Metres are filtered with their speed in mm/s, so
# that one beta serves metres and pixels alike
HAND_STREAMS = (('mesh_xyz', 778, 3, 1000.0), ('joint_xyz', 21, 3, 1000.0), ('joints_px', 21, 2, 1.0), ('camera_px', 3, 1, 1.0))
STREAMS = tuple((n + '_' + s, p, d, v) for s in SIDES for n, p, d, v in HAND_STREAMS) + (('offset', 1, 3, 1000.0),)


class PredictionSmoother(object):
    """One stage of DirEngine.forward, smoothed in FRAME space (the crop moves from frame to frame; the frame does not).

        sm = PredictionSmoother(batch, size=256, fps=30, ...)          # the parameters of OneEuro
        fr = sm.step(stage, M, valid=None)                               # one torch.cat, one launch
        st = sm.crop_stage()                                             # the smoothed values in the crop M, as a stage dict

    Per hand: pd_mesh_xyz (778 points x 3) and pd_joint_xyz (21 x 3) in metres, to_frame_pixels(pd_joint_uv) (21 x 2) in pixels,
    frame_camera(pd_proj) as three scalars (scale_px, trans_px x, y); plus pd_offset (1 x 3).  `fr` holds the smoothed float32 tensors
    'mesh_xyz_left' [B,778,3], 'joint_xyz_left' [B,21,3], 'joints_px_left' [B,21,2], 'camera_px_left' [B,3] (likewise right), 'offset' [B,3],
    'updated' int32 [B], and 'raw': the same streams before the filter.  crop_stage(M) -> pd_mesh_xyz_*, pd_joint_xyz_*, pd_offset as
    smoothed, pd_joint_uv_* = from_frame_pixels, pd_proj_* = crop_camera.  With the step's own M (the default), a row the filter passed
    through or initialised (y = x) gets the stage's own values: mapping to frame pixels and back rounds twice."""

    def __init__(self, batch, size=256, device='cuda', **params):
        self.size = int(size)
        self.filter = OneEuro([(p, d, v) for _, p, d, v in STREAMS], batch, device=device, **params)
        self._last = None

    @staticmethod
    def _split(flat):
        out, at, B = {}, 0, flat.shape[0]
        for name, p, d, _ in STREAMS:
            t = flat[:, at:at + p * d]
            out[name] = t.reshape(B, p, d) if p > 1 and d > 1 else t
            at += p * d
        return out

    def pack(self, stage, M):
        """-> float32 [B,F]: the frame-space streams of a stage, in STREAMS' order"""
        parts = []
        for s in SIDES:
            sc, tr = CR.frame_camera(stage['pd_proj_' + s].float(), M, self.size)
            parts += [stage['pd_mesh_xyz_' + s].float().flatten(1), stage['pd_joint_xyz_' + s].float().flatten(1),
                      CR.to_frame_pixels(stage['pd_joint_uv_' + s].float(), M, self.size).flatten(1), sc[:, None], tr]
        parts.append(stage['pd_offset'].float().flatten(1))
        return torch.cat(parts, 1)

    def step(self, stage, M, valid=None):
        x = self.pack(stage, M)
        y, updated = self.filter.step(x, valid)
        fr = self._split(y)
        fr['updated'], fr['raw'] = updated, self._split(x)
        self._last = (fr, stage, M)
        return fr

    def crop_stage(self, M=None):
        if self._last is None:
            raise ValueError('PredictionSmoother.crop_stage: no step yet')
        fr, stage, M0 = self._last
        own = M is None or M is M0
        M = M0 if M is None else M
        B = fr['offset'].shape[0]
        keep = (fr['updated'] != UPDATED) if own else None

        def pick(new, key):
            raw = stage[key].float().reshape(new.shape)
            return new.contiguous() if keep is None else torch.where(keep.reshape((B,) + (1,) * (new.dim() - 1)), raw, new)
        out = {'pd_offset': pick(fr['offset'].reshape(stage['pd_offset'].shape), 'pd_offset')}
        for s in SIDES:
            cam = fr['camera_px_' + s]
            out['pd_mesh_xyz_' + s] = pick(fr['mesh_xyz_' + s], 'pd_mesh_xyz_' + s)
            out['pd_joint_xyz_' + s] = pick(fr['joint_xyz_' + s], 'pd_joint_xyz_' + s)
            out['pd_joint_uv_' + s] = pick(CR.from_frame_pixels(fr['joints_px_' + s], M, self.size).float(), 'pd_joint_uv_' + s)
            out['pd_proj_' + s] = pick(CR.crop_camera(cam[:, 0], cam[:, 1:3], M, self.size).float(), 'pd_proj_' + s)
        return out

    def jitter(self):
        """OneEuro.jitter() with the streams' names: {'streams': [names], 'raw', 'filtered', 'frames', 'sums'}"""
        return dict(self.filter.jitter(), streams=[n for n, _, _, _ in STREAMS])


def box_filter(batch, **params):
    """the OneEuro of --smooth_box: (mid_x, mid_y, L) of the tracked box as three scalar points, in pixels"""
    return OneEuro([(3, 1, 1.0)], batch, **params)


def smooth_matrices(filt, M_next, ok, size=256):
    """The next tracked box through `filt` (box_filter) before the next crop is made.  M_next float64 [B,6], ok int32 [B]:
    crop_matrices_from_meshes' results.  (mid_x, mid_y, L) come out of M_next by cut_img's formula read backwards (L = size / 2 / s,
    mid = L - t / s, float64), go through the filter as float32 with valid = ok -- a held box does not touch the state -- and the matrix
    is rebuilt in float64: s = (size / 2) / L, M = [[s, 0, s (L - mid_x)], [0, s, s (L - mid_y)]].  Where the filter initialised (a first
    box) or passed the row through, the result is M_next itself, bit for bit.  No host read.  -> (M float64 [B,6], updated int32 [B])"""
    half = float(size) / 2.0
    s = M_next[:, 0]
    L = half / s
    box = torch.stack((L - M_next[:, 2] / s, L - M_next[:, 5] / s, L), 1).float().contiguous()
    y, updated = filt.step(box, ok.contiguous())
    yd = y.double()
    s2 = half / yd[:, 2]
    z = torch.zeros_like(s2)
    M = torch.stack((s2, z, s2 * (yd[:, 2] - yd[:, 0]), z, s2, s2 * (yd[:, 2] - yd[:, 1])), 1)
    return torch.where((updated == UPDATED)[:, None], M, M_next).contiguous(), updated
