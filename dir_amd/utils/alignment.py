"""Aligned evaluation measures on the GPU: csrc/alignmetric.hip through dir_procrustes_align, dir_point_set_nn and dir_threshold_counts.
The reference reports root-relative errors scaled by bone length only; these are the numbers most hand-reconstruction tables carry:

  PA-MPJPE / PA-MPVPE  the mean joint / vertex error after the best similarity alignment of the prediction onto the ground truth
                       (Umeyama 1991; the rotation is always proper -- FreiHAND's script lets a reflection through), in mm
  PCK / AUC            the share of points with an error of at most t, for t over 0 .. 50 mm, and trapz(PCK, t) / 50 mm
  F@5 / F@15           per sample: P = the share of aligned predicted vertices within tau of their nearest ground-truth vertex, R = the same
                       for the ground-truth vertices, F = 2PR / (P + R) (0 when P + R = 0); then the mean over the samples (FreiHAND)

The rules are written out in csrc/alignmetric.hip and restated in float64 numpy by tests/helpers/alignment_ref.py.

  procrustes_align   pd, gt [B,N,3] -> {'err' [B,N], 'transform' [B,13] (s, R row-major, t), 'aligned' [B,N,3] on request}, device tensors
  nn_distances       a [B,Na,3], b [B,Nb,3] -> (d_ab [B,Na], d_ba [B,Nb])
  threshold_counts   err, thresholds [K] -> counts int64 [K+1], ADDED to `counts` when one is given
  pck_auc            counts, thresholds -> (PCK curve, AUC), on the host
  AlignedMetrics     the accumulator beside apps.eval.EvalMetrics: update / arrays / summarize / report / save_txt
"""
import os

import numpy as np
import torch

from .. import _capi

ALIGN_SCALE = 1                            # DIR_ALIGN_SCALE
MAX_THRESHOLDS = 1024                      # DIR_ALIGN_MAX_THRESHOLDS
F_TAUS = (0.005, 0.015)                    # metres
SIDES = ('left', 'right')


def default_thresholds():
    return np.linspace(0, 0.05, 100)


def _sets(what, a, b, same_n):
    _capi.require_cuda(a, b)
    a, b = _capi.f32c(a), _capi.f32c(b)
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0] or a.shape[0] == 0 or \
            (same_n and a.shape[1] != b.shape[1]) or a.device != b.device:
        raise ValueError('%s: need two point sets [B,N,3] of one non-empty batch on one device, got %s and %s' % (what, tuple(a.shape), tuple(b.shape)))
    return a, b


def procrustes_align(pd, gt, scale=True, want_aligned=False):
    """dir_procrustes_align: the similarity that maps each pd[b] onto gt[b] in the least-squares sense.  -> {'err' [B,N] = |aligned - gt|,
    'transform' [B,13] = s, R row-major, t; with want_aligned also 'aligned' [B,N,3] = s R pd + t}.  A sample with a non-finite
    coordinate or with all of pd's points equal is NaN throughout."""
    pd, gt = _sets('procrustes_align', pd, gt, True)
    B, N, dev = pd.shape[0], pd.shape[1], pd.device
    out = {'err': torch.empty(B, N, device=dev), 'transform': torch.empty(B, 13, device=dev)}
    if want_aligned:
        out['aligned'] = torch.empty(B, N, 3, device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_procrustes_align(P(pd), P(gt), B, N, ALIGN_SCALE if scale else 0, P(out['transform']), P(out.get('aligned')),
                                                     P(out['err']), _capi.stream_ptr()), 'dir_procrustes_align')
    return out


def nn_distances(a, b):
    """dir_point_set_nn: -> (d_ab [B,Na], d_ba [B,Nb]), the distance from each point of one set to the nearest point of the other"""
    a, b = _sets('nn_distances', a, b, False)
    B, dev = a.shape[0], a.device
    d_ab, d_ba = torch.empty(B, a.shape[1], device=dev), torch.empty(B, b.shape[1], device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().dir_point_set_nn(P(a), P(b), B, a.shape[1], b.shape[1], P(d_ab), P(d_ba), _capi.stream_ptr()), 'dir_point_set_nn')
    return d_ab, d_ba


def threshold_counts(err, thresholds, counts=None):
    """dir_threshold_counts: err any shape, thresholds float32 [K] on the GPU -> counts int64 [K+1]: counts[k] = the finite values <=
    thresholds[k], counts[K] = the finite values.  With `counts` given (int64 [K+1], contiguous) the numbers are added to it."""
    _capi.require_cuda(err, thresholds, counts)
    err, thresholds = _capi.f32c(err), _capi.f32c(thresholds)
    K = thresholds.numel()
    if thresholds.dim() != 1 or err.numel() == 0:
        raise ValueError('threshold_counts: need values and thresholds [K], got %s and %s' % (tuple(err.shape), tuple(thresholds.shape)))
    if counts is None:
        counts = torch.zeros(K + 1, dtype=torch.int64, device=err.device)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (K + 1,) or not counts.is_contiguous() or counts.device != err.device:
        raise ValueError('threshold_counts: counts must be a contiguous int64 [%d] on %s' % (K + 1, err.device))
    P = _capi.ptr
    with torch.cuda.device(err.device):
        _capi.check(_capi.lib().dir_threshold_counts(P(err), err.numel(), P(thresholds), K, P(counts), _capi.stream_ptr()), 'dir_threshold_counts')
    return counts


def pck_auc(counts, thresholds):
    """counts [K+1] (threshold_counts), thresholds [K] ascending, on the host -> (PCK [K], AUC = trapz(PCK, t) / (t[-1] - t[0]))"""
    c, t = np.asarray(counts, np.float64), np.asarray(thresholds, np.float64)
    if not c[-1]:
        return np.full(len(t), np.nan), float('nan')
    y = c[:-1] / c[-1]
    return y, float(((y[1:] + y[:-1]) / 2 * np.diff(t)).sum() / (t[-1] - t[0]))


_CURVES = ('pa_joint', 'pa_vert', 'joint')          # aligned joints, aligned vertices, the unaligned root-relative joints of eval_batch
_KEEP = ('err_joint', 'err_vert', 'near')


class AlignedMetrics:
    """The accumulator beside apps.eval.EvalMetrics.  J_regressor = {'left': Jr, 'right': Jr}; thresholds: ascending, metres (default
    linspace(0, 0.05, 100)).  update() scores the last stage of a batch, each hand alone: joints = Jr(vertices) for prediction and
    ground truth, both taken raw (the alignment subsumes root and scale); joints are aligned on joints, vertices on vertices, with
    scale; the aligned vertices and the ground truth's give the nearest-neighbour distances of the F-scores.  A hand whose joint or
    vertex alignment is NaN is counted as `invalid` and enters nothing.  Per-sample results stay on the GPU until summarize() /
    save_txt(), which read them once."""

    def __init__(self, J_regressor, stage_num=3, thresholds=None, root_joint=0, scale=True):
        t = np.asarray(default_thresholds() if thresholds is None else thresholds, np.float64).reshape(-1)
        if not 2 <= len(t) <= MAX_THRESHOLDS or not (np.diff(t) > 0).all():
            raise ValueError('AlignedMetrics: need 2..%d ascending thresholds' % MAX_THRESHOLDS)
        self.J_regressor, self.stage_num, self.thresholds, self.root_joint, self.scale = J_regressor, stage_num, t, root_joint, scale
        self.batches = []
        # made here, on the caller's stream, before any update: the slots' streams of evaluate_from_disk all add to `counts`, and each of them
        # is ordered after this zero fill by the event it waits for before its update
        dev = J_regressor['left'].J_regressor.device
        self.counts = torch.zeros(2, len(_CURVES), len(t) + 1, dtype=torch.int64, device=dev)          # [hand, curve, K+1]
        self._thr = torch.from_numpy(t.astype(np.float32)).to(dev)
        self._taus = torch.tensor(F_TAUS, dtype=torch.float32).to(dev)
        self._nan = torch.full((), float('nan')).to(dev)
        self._arrays = None

    def update(self, result, data, eval_out=None):
        """`result` = network(...)[0]; `data` = the dataloader tuple of apps/eval.py:139-149 (data[3] / data[5]: the ground-truth meshes;
        data[7], data[9], data[10] are read only when eval_out is not given); eval_out: eval_batch's dict for this batch, if the caller
        has it already (its 'joint_err' gives the unaligned curve)."""
        from ..apps.eval import eval_batch
        r = result[self.stage_num - 1]
        pd = {s: _capi.f32c(r['pd_mesh_xyz_' + s]) for s in SIDES}
        gt = {'left': _capi.f32c(data[3].cuda()), 'right': _capi.f32c(data[5].cuda())}
        if eval_out is None:
            eval_out = eval_batch(self.J_regressor, pd, r['pd_offset'], gt, {'left': data[7].cuda(), 'right': data[9].cuda()}, data[10].cuda(),
                                  self.root_joint, self.scale)
        nan = self._nan
        out = {}
        for h, s in enumerate(SIDES):
            jr = self.J_regressor[s]
            ej = procrustes_align(jr(pd[s]), jr(gt[s]))['err']
            av = procrustes_align(pd[s], gt[s], want_aligned=True)
            d_pd, d_gt = nn_distances(av['aligned'], gt[s])
            valid = ~(torch.isnan(ej[:, 0]) | torch.isnan(av['err'][:, 0]))
            ej, ev = torch.where(valid[:, None], ej, nan), torch.where(valid[:, None], av['err'], nan)
            ju = torch.where(valid[:, None], eval_out['joint_err'][:, h], nan).contiguous()
            for c, e in enumerate((ej, ev, ju)):
                threshold_counts(e, self._thr, self.counts[h, c])
            # vertices nearer than tau, per sample: [B, tau, (predicted, ground truth)]; integers, so any order of summation gives them
            near = torch.stack([(d_pd[:, None, :] < self._taus[None, :, None]).sum(2), (d_gt[:, None, :] < self._taus[None, :, None]).sum(2)], 2)
            out[s] = {'err_joint': ej, 'err_vert': ev, 'near': near.to(torch.int32)}
        self.batches.append(out)
        self._arrays = None
        return out

    def arrays(self):
        """{'left' / 'right': {'err_joint' [n,21], 'err_vert' [n,V] (metres, NaN rows: invalid), 'near' int [n,2,2], 'valid' bool [n]},
        'counts' int64 [2,3,K+1]} as numpy arrays; one host read"""
        if not self.batches:
            raise ValueError('AlignedMetrics: no batch was scored')
        if self._arrays is None:
            a = {s: {k: torch.cat([b[s][k] for b in self.batches], 0).cpu().numpy() for k in _KEEP} for s in SIDES}
            for s in SIDES:
                a[s]['valid'] = ~np.isnan(a[s]['err_joint'][:, 0])
            a['counts'] = self.counts.cpu().numpy()
            self._arrays = a
        return self._arrays

    def f_scores(self, side):
        """[n,2] float64: F@5 mm and F@15 mm per sample (NaN: invalid)"""
        a = self.arrays()[side]
        nv = a['err_vert'].shape[1]
        P, R = a['near'][:, :, 0] / np.float64(nv), a['near'][:, :, 1] / np.float64(nv)
        with np.errstate(divide='ignore', invalid='ignore'):
            f = np.where(P + R > 0, 2 * P * R / (P + R), 0.0)
        f[~a['valid']] = np.nan
        return f

    def summarize(self):
        a, s = self.arrays(), {}
        per = {}
        for h, side in enumerate(SIDES):
            v = a[side]['valid']
            f = self.f_scores(side)[v]
            d = {'pa_mpjpe_mm': float(a[side]['err_joint'][v].astype(np.float64).mean() * 1000) if v.any() else float('nan'),
                 'pa_mpvpe_mm': float(a[side]['err_vert'][v].astype(np.float64).mean() * 1000) if v.any() else float('nan'),
                 'f_5': float(f[:, 0].mean()) if v.any() else float('nan'), 'f_15': float(f[:, 1].mean()) if v.any() else float('nan')}
            for c, name in enumerate(_CURVES):
                d['pck_' + name], d['auc_' + name] = pck_auc(a['counts'][h, c], self.thresholds)
            d['samples'], d['invalid'] = int(v.sum()), int((~v).sum())
            per[side] = d
        for k in ('pa_mpjpe_mm', 'pa_mpvpe_mm', 'f_5', 'f_15') + tuple('auc_' + c for c in _CURVES):
            l, r = per['left'][k], per['right'][k]
            s[k] = {'left': l, 'right': r, 'all': (l + r) / 2}
        for c in _CURVES:
            s['pck_' + c] = {side: per[side]['pck_' + c] for side in SIDES}
        s['samples'] = {side: per[side]['samples'] for side in SIDES}
        s['invalid'] = {side: per[side]['invalid'] for side in SIDES}
        return s

    def report(self):
        s = self.summarize()
        lines = ['aligned (per-hand similarity alignment, proper rotations only):']
        for title, key, unit in (('PA-MPJPE:', 'pa_mpjpe_mm', ' mm'), ('PA-MPVPE:', 'pa_mpvpe_mm', ' mm'),
                                 ('AUC of PCK over 0-{} mm, aligned joints:'.format(self.thresholds[-1] * 1000), 'auc_pa_joint', ''),
                                 ('AUC, aligned vertices:', 'auc_pa_vert', ''), ('AUC, root-relative joints (not aligned):', 'auc_joint', ''),
                                 ('F@5 mm:', 'f_5', ''), ('F@15 mm:', 'f_15', '')):
            lines.append('    {} left: {}{u}, right: {}{u}, all: {}{u}'.format(title, s[key]['left'], s[key]['right'], s[key]['all'], u=unit))
        if s['invalid']['left'] or s['invalid']['right']:
            lines.append('    hands left out (no alignment exists): left {}, right {}'.format(s['invalid']['left'], s['invalid']['right']))
        return '\n'.join(lines)

    def save_txt(self, file_folder):
        """pa_joint_{left,right}_error.txt [n,21] and pa_mesh_{left,right}_error.txt [n] (mm), fscore.txt [n,4] (F@5 left, F@15 left, F@5
        right, F@15 right), pck.txt [K,7] (the threshold in mm; aligned joints, aligned vertices, unaligned joints for the left hand, then
        the right)"""
        os.makedirs(file_folder, exist_ok=True)
        a, s = self.arrays(), self.summarize()
        w = lambda n, x, fmt='%.3f': np.savetxt(os.path.join(file_folder, n), x, fmt=fmt)  # noqa: E731
        for side in SIDES:
            w('pa_joint_%s_error.txt' % side, a[side]['err_joint'].astype(np.float64) * 1000)
            w('pa_mesh_%s_error.txt' % side, a[side]['err_vert'].astype(np.float64).mean(-1) * 1000)
        w('fscore.txt', np.concatenate([self.f_scores('left'), self.f_scores('right')], 1), '%.6f')
        w('pck.txt', np.stack([self.thresholds * 1000] + [s['pck_' + c][side] for side in SIDES for c in _CURVES], 1), '%.6f')
