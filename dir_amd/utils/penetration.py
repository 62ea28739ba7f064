"""Inter-hand penetration of predicted (or ground-truth) meshes on the GPU: csrc/penetration.hip through dir_mesh_penetration and
dir_mesh_intersection_volume.  The reference sets up `inter_volume_list` (apps/eval.py:134) and never fills it; these are the measures
it would have reported, by the usual definitions (ObMan, Hasson et al. 2019):

  penetration depth    the largest distance from a vertex of one mesh that lies inside the other mesh to that mesh's surface
  intersection volume  the volume shared by both meshes, counted on a voxel lattice (5 mm by default)

A point p is inside a mesh when |w(p)| > 0.5, w the generalised winding number (independent of the face orientation, tolerant of MANO's
open wrist); the distance is to the closest point of the closed triangles; a face with a repeated index or an index outside 0..V-1 is
skipped.  The rules are written out in csrc/penetration.hip and restated in float64 numpy by tests/helpers/penetration_ref.py.

  mesh_penetration      two batched meshes -> per direction count / max_depth / sum_depth (+ per-vertex winding / dist), device tensors
  intersection_volume   two batched meshes -> volume / n_both / cells, device tensors
  close_boundary        host: faces + a fan over their single boundary loop (MANO's wrist), no new vertex
  hand_faces            two_hand_faces' [3076,3] table -> the (left, right) tables the kernels take, optionally sealed
  two_hand_penetration  one stage of DIR.forward -> both measures, the hands placed in their common frame
  PenetrationMetrics    the accumulator beside apps.eval.EvalMetrics: update / update_gt / summarize / report / save_txt
"""
import os

import numpy as np
import torch

from .. import _capi

MAX_VERTS, MAX_FACES = 4096, 8192          # DIR_MESH_MAX_VERTS / DIR_MESH_MAX_FACES
OFFSET_UNIT = 0.15                         # pd_offset is in units of 0.15 m (apps/eval.py:170)


def _meshes(what, verts_a, faces_a, verts_b, faces_b):
    _capi.require_cuda(verts_a, faces_a, verts_b, faces_b)
    va, vb = _capi.f32c(verts_a), _capi.f32c(verts_b)
    for v, f in ((va, faces_a), (vb, faces_b)):
        if v.dim() != 3 or v.shape[2] != 3 or f.dim() != 2 or f.shape[1] != 3 or f.dtype != torch.int32 or not f.is_contiguous():
            raise ValueError('%s: need float vertices [B,V,3] and contiguous int32 faces [F,3], got %s and %s %s'
                             % (what, tuple(v.shape), f.dtype, tuple(f.shape)))
    if va.shape[0] != vb.shape[0] or va.shape[0] == 0:
        raise ValueError('%s: the meshes need one non-empty batch, got %d and %d samples' % (what, va.shape[0], vb.shape[0]))
    return va, vb


def mesh_penetration(verts_a, faces_a, verts_b, faces_b, per_vertex=False):
    """dir_mesh_penetration: verts_a [B,Va,3], faces_a int32 [Fa,3], verts_b [B,Vb,3], faces_b int32 [Fb,3] on the GPU, both meshes in one
    frame.  Direction 0 = A's vertices inside B, direction 1 = B's inside A.  -> {'count' int32 [B,2], 'max_depth' [B,2] (metres),
    'sum_depth' [B,2], 'depth' [B]: the sample's penetration depth, the larger max_depth}; with per_vertex also 'winding' and 'dist'
    [B,Va+Vb], A's vertices first, each against the other mesh."""
    va, vb = _meshes('mesh_penetration', verts_a, faces_a, verts_b, faces_b)
    B, dev = va.shape[0], va.device
    out = {'count': torch.empty(B, 2, dtype=torch.int32, device=dev), 'max_depth': torch.empty(B, 2, device=dev),
           'sum_depth': torch.empty(B, 2, device=dev)}
    if per_vertex:
        out['winding'] = torch.empty(B, va.shape[1] + vb.shape[1], device=dev)
        out['dist'] = torch.empty_like(out['winding'])
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_mesh_penetration(P(va), P(faces_a), P(vb), P(faces_b), B, va.shape[1], faces_a.shape[0], vb.shape[1],
                                                     faces_b.shape[0], P(out.get('winding')), P(out.get('dist')), P(out['count']),
                                                     P(out['max_depth']), P(out['sum_depth']), _capi.stream_ptr()), 'dir_mesh_penetration')
    out['depth'] = out['max_depth'].amax(1)
    return out


def intersection_volume(verts_a, faces_a, verts_b, faces_b, pitch=0.005, max_cells=1 << 17):
    """dir_mesh_intersection_volume: the meshes as mesh_penetration takes them; the lattice (i, j, k) * pitch over the intersection of
    the two bounding boxes.  -> {'volume' [B] (cubic metres; NaN where the lattice has more than max_cells points: nothing is examined
    then), 'n_both' int32 [B], 'cells' int32 [B]}.  Nothing is read back: the launch does not depend on the boxes."""
    va, vb = _meshes('intersection_volume', verts_a, faces_a, verts_b, faces_b)
    B, dev = va.shape[0], va.device
    out = {'volume': torch.empty(B, device=dev), 'n_both': torch.empty(B, dtype=torch.int32, device=dev),
           'cells': torch.empty(B, dtype=torch.int32, device=dev)}
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_mesh_intersection_volume(P(va), P(faces_a), P(vb), P(faces_b), B, va.shape[1], faces_a.shape[0],
                                                             vb.shape[1], faces_b.shape[0], float(pitch), int(max_cells), P(out['volume']),
                                                             P(out['n_both']), P(out['cells']), _capi.stream_ptr()),
                    'dir_mesh_intersection_volume')
    return out


def close_boundary(faces):
    """faces int [F,3] (host) -> int32 [F+n,3]: the faces plus a fan over their boundary, with no new vertex.  The boundary edges (used by
    exactly one face) must form a single simple loop of n + 2 vertices -- real MANO has one, at the wrist; each fan triangle runs along
    its boundary edge in the opposite direction to the face beside it, so every edge ends up with two faces of opposite direction.
    Anything else (no boundary, several loops, a vertex on more than two boundary edges, an edge used by three faces): ValueError."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError('close_boundary: need integer faces [F,3], got %s %s' % (f.dtype, f.shape))
    f = f.astype(np.int64)
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
        raise ValueError('close_boundary: a face repeats a vertex index')
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])          # directed edges, as the faces run along them
    key = np.sort(e, 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    if cnt.max() > 2:
        raise ValueError('close_boundary: an edge is used by %d faces' % cnt.max())
    b = e[cnt[inv.reshape(-1)] == 1]
    if len(b) < 3:
        raise ValueError('close_boundary: the faces have no boundary loop (%d boundary edges)' % len(b))
    nxt = {}
    for u, v in b:
        if int(u) in nxt:
            raise ValueError('close_boundary: vertex %d starts two boundary edges: the boundary is not a simple loop' % u)
        nxt[int(u)] = int(v)
    if sorted(nxt) != sorted(nxt.values()):
        raise ValueError('close_boundary: the boundary edges do not chain into loops')
    loop = [int(b[0, 0])]
    while nxt[loop[-1]] != loop[0]:
        loop.append(nxt[loop[-1]])
        if len(loop) > len(b):
            raise ValueError('close_boundary: the boundary is not a simple loop')
    if len(loop) != len(b):
        raise ValueError('close_boundary: %d boundary edges form more than one loop (the first has %d)' % (len(b), len(loop)))
    # the faces run loop[i] -> loop[i+1]; the fan (loop[0], loop[i+1], loop[i]) runs every boundary edge backwards, and its own inner
    # edges once in each direction
    fan = np.array([[loop[0], loop[i + 1], loop[i]] for i in range(1, len(loop) - 1)], np.int64)
    return np.ascontiguousarray(np.concatenate([f, fan]).astype(np.int32))


def hand_faces(table, seal='off', device='cuda'):
    """vis_utils.two_hand_faces' table ([2F,3]: the left hand's faces, then the right hand's with 778 added) -> (left, right) int32 cuda
    tables, the right one re-based to 0.  seal: 'on' closes each hand's boundary loop (close_boundary; ValueError when there is none),
    'auto' does when both hands have one, 'off' leaves the tables as they are.  -> (left, right, sealed)."""
    from .vis_utils import NV_HAND
    t = np.asarray(table.cpu() if torch.is_tensor(table) else table)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] % 2 or seal not in ('auto', 'on', 'off'):
        raise ValueError("hand_faces: need a [2F,3] table and seal in 'auto' / 'on' / 'off', got %s, %r" % (t.shape, seal))
    half = t.shape[0] // 2
    left, right = t[:half].astype(np.int64), t[half:].astype(np.int64) - NV_HAND
    sealed = False
    if seal != 'off':
        try:
            left, right, sealed = close_boundary(left), close_boundary(right), True
        except ValueError:
            if seal == 'on':
                raise
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(device)  # noqa: E731
    return to(left), to(right), sealed


def two_hand_penetration(stage, faces, volume_pitch=None, max_cells=1 << 17):
    """One stage dict of DIR.forward -> mesh_penetration's dict for (A = left hand, B = right hand), plus intersection_volume's when
    volume_pitch is a positive number.  The hands are placed in the frame apps/eval.py:170,236-238 implies: the left vertices are
    pd_mesh_xyz_left, the right ones pd_mesh_xyz_right + 0.15 * pd_offset.  faces: hand_faces' (left, right) pair, or two_hand_faces'
    [3076,3] table (its right half is re-based to 0 here, on every call)."""
    if not isinstance(faces, (tuple, list)):
        faces = hand_faces(faces, device=stage['pd_mesh_xyz_left'].device)
    fl, fr = faces[0], faces[1]
    left = _capi.f32c(stage['pd_mesh_xyz_left'])
    right = _capi.f32c(stage['pd_mesh_xyz_right']) + OFFSET_UNIT * _capi.f32c(stage['pd_offset'])[:, None, :]
    out = mesh_penetration(left, fl, right, fr)
    if volume_pitch:
        out.update(intersection_volume(left, fl, right, fr, pitch=volume_pitch, max_cells=max_cells))
    return out


_KEYS = ('count', 'depth', 'sum_depth', 'volume')


class PenetrationMetrics:
    """The accumulator beside apps.eval.EvalMetrics.  faces: hand_faces' pair (or two_hand_faces' table); volume_pitch: the lattice
    pitch in metres, None / 0 = no volume.  Per-sample results stay on the GPU until summarize() / save_txt(), which read them once."""

    def __init__(self, faces, stage_num=3, volume_pitch=0.005, max_cells=1 << 17):
        self.faces, self.stage_num, self.volume_pitch, self.max_cells = faces, stage_num, volume_pitch or None, max_cells
        self.batches, self.gt_batches = [], []
        self._arrays = None

    def _keep(self, out):
        if 'volume' not in out:
            out['volume'] = torch.full_like(out['depth'], float('nan'))
        self._arrays = None
        return {k: out[k] for k in _KEYS}

    def update(self, result):
        """`result` = network(...)[0] (the list of stage dicts)"""
        out = two_hand_penetration(result[self.stage_num - 1], self.faces, self.volume_pitch, self.max_cells)
        self.batches.append(self._keep(out))
        return out

    def update_gt(self, data):
        """`data` = the dataloader tuple of apps/eval.py:139-149: data[3] / data[5] are the ground-truth meshes, already in one frame"""
        if not isinstance(self.faces, (tuple, list)):
            self.faces = hand_faces(self.faces, device='cuda')
        left, right = data[3].cuda(), data[5].cuda()
        out = mesh_penetration(left, self.faces[0], right, self.faces[1])
        if self.volume_pitch:
            out.update(intersection_volume(left, self.faces[0], right, self.faces[1], pitch=self.volume_pitch, max_cells=self.max_cells))
        self.gt_batches.append(self._keep(out))
        return out

    def arrays(self, gt=False):
        """{'count' [N,2], 'depth' [N], 'sum_depth' [N,2], 'volume' [N]} as numpy arrays (metres, cubic metres); one host read"""
        if self._arrays is None:
            self._arrays = [None if not bs else {k: v.cpu().numpy() for k, v in {k: torch.cat([b[k] for b in bs], 0) for k in _KEYS}.items()}
                            for bs in (self.batches, self.gt_batches)]
        a = self._arrays[1 if gt else 0]
        if a is None:
            raise ValueError('PenetrationMetrics: no %s batch was scored' % ('ground-truth' if gt else 'predicted'))
        return a

    def summarize(self, gt=False):
        a = self.arrays(gt)
        n_in = a['count'].sum(1).astype(np.float64)
        vol = a['volume'].astype(np.float64)
        known = np.isfinite(vol)
        return {'depth_mean_mm': float(a['depth'].astype(np.float64).mean() * 1000),
                'depth_max_mm': float(a['depth'].max() * 1000),
                'vertex_depth_mean_mm': float(a['sum_depth'].astype(np.float64).sum() / n_in.sum() * 1000) if n_in.sum() else 0.0,
                'rate': float((n_in > 0).mean()),
                'vertices_mean': float(n_in.mean()),
                'volume_mean_cm3': float(vol[known].mean() * 1e6) if known.any() else float('nan'),
                'volume_unknown': int((~known).sum()) if self.volume_pitch else 0,
                'samples': int(len(n_in))}

    def report(self, gt=False):
        s = self.summarize(gt)
        lines = ['%spenetration:' % ('ground-truth ' if gt else ''),
                 '    depth: mean {} mm, max {} mm'.format(s['depth_mean_mm'], s['depth_max_mm']),
                 '    over penetrating vertices: mean depth {} mm'.format(s['vertex_depth_mean_mm']),
                 '    samples with penetration: {} %, penetrating vertices per sample: {}'.format(100 * s['rate'], s['vertices_mean'])]
        if self.volume_pitch:
            lines.append('    intersection volume ({} mm lattice): mean {} cm^3{}'.format(
                self.volume_pitch * 1000, s['volume_mean_cm3'],
                ' ({} samples over {} lattice points left out)'.format(s['volume_unknown'], self.max_cells) if s['volume_unknown'] else ''))
        return '\n'.join(lines)

    def rows(self, gt=False):
        """[N,4] float64: left-in-right count, right-in-left count, depth in mm, volume in cm^3 (nan: not computed)"""
        a = self.arrays(gt)
        return np.concatenate([a['count'].astype(np.float64), a['depth'].astype(np.float64)[:, None] * 1000,
                               a['volume'].astype(np.float64)[:, None] * 1e6], 1)

    def save_txt(self, file_folder):
        """penetration.txt (and penetration_gt.txt when update_gt ran): one row per image, as rows()"""
        os.makedirs(file_folder, exist_ok=True)
        np.savetxt(os.path.join(file_folder, 'penetration.txt'), self.rows(), fmt=['%d', '%d', '%.3f', '%.3f'])
        if self.gt_batches:
            np.savetxt(os.path.join(file_folder, 'penetration_gt.txt'), self.rows(True), fmt=['%d', '%d', '%.3f', '%.3f'])
