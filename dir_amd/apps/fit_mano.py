"""MANO parameters for hands that come without them: 3-D joints, meshes (a dataset's, or another model's output) or 2-D keypoints -> the
64-vector of this tree (6D root, 45 PCA coefficients, 10 betas, 3 camera scalars), fitted on the GPU by dir_mano_fit (utils/mano_fit.py).

    python -m dir_amd.apps.fit_mano --model CKPT --targets T.npz --out O.npz [--iters 200] [--lr 0.1] [--lr_root --lr_pca --lr_betas --lr_cam]
                                    [--bs 256] [--center 0] [--cam_scale 1.0] [--w_verts 1e4 --w_joints 1e4 --w_uv 1 --w_pca 0 --w_beta 0
                                    --w_init 0] [--ema] [--start neutral|closed] [--sequences [--w_t_root 1 --w_t_pca 1 --w_t_cam 1] [--per_frame_shape]]
                                    [--pair [--w_col 1e4 --w_offset 0 --w_offset_init 0 --lr_offset LR --radii FILE|auto]]

The MANO tables come from the checkpoint (init_regressor.mano_layer_{left,right}.th_*), as in apps.predict.  T.npz holds, per side in
(left, right), any of  verts_<side> [N,778,3],  joints_<side> [N,21,3] with joints_conf_<side> [N,21],  joint_uv_<side> [N,21,2] (the crop's
-1..1 coordinates, as pd_joint_uv_*) with uv_conf_<side> [N,21],  and optionally init_<side> [N,64] (default: neutral_para(N, --cam_scale)).
3-D targets are relative to joint --center of the same hand (joint order of pd_joint_xyz_*; -1: not centred); a confidence of 0 drops an
entry, which may then hold NaN.  A side with no target is left out.  O.npz holds para_<side> [N,64], the fitted verts_ / joints_ / joint_uv_<side>,
mse_before_<side> and mse_after_<side> [N,3] (mean squared residual of the vertices, 3-D joints and 2-D joints, unweighted) and status_<side>
[N] (bit 0 reflection, bit 1 non-finite input: passed through, bit 2 a step went non-finite: stopped there).  The last line printed is
"N hands in T s".  --start closed (default neutral: the output is as without the flag): before the fit, dir_mano_fit_start turns the start's root onto 3-D
targets by a rigid alignment (with 2-D targets alone: the best of the cube's 24 rotations) and fits its camera by least squares
(utils/mano_fit.py start_mano), so targets rotated anywhere are reached and --cam_scale need not be guessed; the fit is anchored at the started
parameters, and O.npz gains start_<side> [N,64], start_status_<side> [N] (8: the root was kept, 16: the camera was kept) and start_choice_<side>
[N] (the rotation the 2-D search wrote, else -1).  The defaults are NOT tuned on real MANO tables or real keypoints.

--sequences: the N hands of a side are the frames of S sequences laid end to end, T.npz carries seq_len [S] (ints >= 1 summing to N; both sides share
it), and ONE optimisation runs over each batch of whole sequences (dir_mano_fit_sequence, utils/mano_fit.py fit_mano_sequence): one shape per
(sequence, side) unless --per_frame_shape, and the temporal term --w_t_root / --w_t_pca / --w_t_cam between neighbouring frames, which fills a frame
whose confidences are all 0 from its neighbours.  A batch takes whole sequences up to --bs frames (a longer sequence is a batch of its own).  O.npz gains
betas_<side> [S,10] (the sequence's shape: para_<side>'s 51:61 of its first frame that did not pass through; NaN where there is none) and
seq_status_<side> [S] (2: no usable frame, 4: the shape was frozen); status_<side> gains bit 3 (a non-finite target in use: the frame's data terms were
dropped).  Without --sequences every byte written is what it is without these flags.  The temporal defaults are NOT tuned on real tracks.

--pair: row n of the left side and row n of the right side are the two hands of one person, fitted TOGETHER (dir_mano_fit_pair, utils/mano_fit.py
fit_mano_pair): the offset o [N,3] between them (right centre joint minus left, metres, camera axes; 0.15 x pd_offset) is a further variable, and a
capsule per bone keeps the hands from passing through each other (--w_col).  T.npz may carry offset [N,3] (the start and, with --w_offset, the target;
default 0) with offset_conf [N]; --w_offset_init pulls o to its start, --lr_offset is its rate (default --lr).  --radii auto: capsule_radii of the
checkpoint's tables; a FILE.npz holds radii_left and radii_right [20].  Both sides need a target and the same N; --center must be >= 0; not with
--sequences.  O.npz gains offset [N,3], collision [N,4] (mean squared and largest capsule overlap in metres before, then after) and pair_status [N]
(1: a hand passed through, 2: offset or radii non-finite -- the coupling was off; 4: the offset was frozen; 8: crossing bones met).  Without --pair
every byte written is what it is without these flags.  The radii quantile and the weights are NOT tuned: this tree has no real MANO tables.
"""
import time

import numpy as np

SIDES = ('left', 'right')
TARGETS = (('verts', (778, 3)), ('joints', (21, 3)), ('joints_conf', (21,)), ('joint_uv', (21, 2)), ('uv_conf', (21,)))


def read_targets(npz):
    """-> {side: {name: float32 array}} for the sides that have a target; ValueError on a wrong shape or a confidence without its target"""
    out = {}
    for side in SIDES:
        d = {}
        for name, shape in TARGETS + (('init', (64,)),):
            k = '%s_%s' % (name, side)
            if k in npz:
                a = np.asarray(npz[k], np.float32)
                if a.ndim != len(shape) + 1 or tuple(a.shape[1:]) != shape:
                    raise ValueError('fit_mano: %s must be [N%s], got %s' % (k, ''.join(',%d' % s for s in shape), list(a.shape)))
                d[name] = a
        if not any(k in d for k in ('verts', 'joints', 'joint_uv')):
            if d:
                raise ValueError('fit_mano: %s has %s but no target (verts, joints or joint_uv)' % (side, sorted(d)))
            continue
        if ('joints_conf' in d and 'joints' not in d) or ('uv_conf' in d and 'joint_uv' not in d):
            raise ValueError('fit_mano: %s has confidences without their target' % side)
        if len({a.shape[0] for a in d.values()}) != 1:
            raise ValueError('fit_mano: the arrays of %s differ in their first dimension' % side)
        out[side] = d
    if not out:
        raise ValueError('fit_mano: the targets hold none of ' + ', '.join('%s_<side>' % n for n in ('verts', 'joints', 'joint_uv')))
    return out


def tables_from_checkpoint(state, center=0, device='cuda'):
    """{side: _capi.ManoTables} from the checkpoint's th_* buffers, and the list that keeps their device tensors alive"""
    import torch  # noqa: F401

    from ..engine import pack_mano
    keep = []
    sd = {k: v.detach().to(device) for k, v in state.items() if k.startswith('init_regressor.mano_layer_')}
    return {s: pack_mano(sd, 'init_regressor.mano_layer_' + s, s, None if center < 0 else center, keep) for s in SIDES}, keep


def sequence_batches(seq_len, bs):
    """whole sequences grouped into batches of at most bs frames (a longer sequence is a batch of its own) -> [(first sequence, one past the last)]"""
    out, s0, n = [], 0, 0
    for s, length in enumerate(seq_len):
        if n and n + length > bs:
            out.append((s0, s))
            s0, n = s, 0
        n += length
    return out + [(s0, len(seq_len))] if len(seq_len) else out


def fit_targets(tables, targets, iters=200, lr=0.1, weights=None, bs=256, cam_scale=1.0, device='cuda', start='neutral', seq_len=None, smooth=None,
                share_betas=True):
    """targets: read_targets' dict -> {side: {para, verts, joints, joint_uv, mse_before, mse_after, status}} (numpy; with start='closed' also start,
    start_status, start_choice).  Both sides with the same N go through one launch per batch as a pair, otherwise one side at a time.
    seq_len (ints [S] summing to every side's N): fit whole sequences (fit_mano_sequence with `smooth` and `share_betas`); the result gains betas [S,10]
    and seq_status [S]."""
    import torch

    from ..utils import mano_fit as MF
    sides = [s for s in SIDES if s in targets]
    n_of = lambda s: next(iter(targets[s].values())).shape[0]  # noqa: E731
    groups = [sides] if len(sides) == 2 and n_of(sides[0]) == n_of(sides[1]) else [[s] for s in sides]
    out = {s: {} for s in sides}
    for grp in groups:
        N = next(iter(targets[grp[0]].values())).shape[0]
        parts = {s: [] for s in grp}
        if seq_len is None:
            spans = [(b0, min(b0 + bs, N), None) for b0 in range(0, N, bs)]
        else:
            if int(np.sum(seq_len)) != N or np.min(seq_len) < 1:
                raise ValueError('fit_mano: seq_len must hold lengths >= 1 that sum to the %d hands of %s' % (N, grp[0]))
            first = np.concatenate([[0], np.cumsum(seq_len)])
            spans = [(int(first[a]), int(first[b]), [int(x) for x in seq_len[a:b]]) for a, b in sequence_batches(seq_len, bs)]
        for b0, b1, lengths in spans:
            dev = lambda s, k: torch.from_numpy(np.ascontiguousarray(targets[s][k][b0:b1])).to(device) if k in targets[s] else None  # noqa: E731
            n = b1 - b0
            arg = lambda k: [dev(s, k) for s in grp] if len(grp) == 2 else dev(grp[0], k)  # noqa: E731
            init = [dev(s, 'init') if 'init' in targets[s] else MF.neutral_para(n, cam_scale, device) for s in grp]
            w = dict(weights or {})
            for k, t in (('w_verts', 'verts'), ('w_joints', 'joints'), ('w_uv', 'joint_uv')):
                if not any(t in targets[s] for s in grp):
                    w[k] = 0.0
                else:
                    w.setdefault(k, MF.DEFAULT_WEIGHTS[k])
            tabs, init = ([tables[s] for s in grp], init) if len(grp) == 2 else (tables[grp[0]], init[0])
            anchor = st = None
            if start == 'closed':
                st = MF.start_mano(tabs, init, arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'), weights=w)
                init = anchor = st.para
            if lengths is None:
                r = MF.fit_mano(tabs, init, arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'), iters=iters, lr=lr, weights=w, anchor=anchor)
            else:
                r = MF.fit_mano_sequence(tabs, init, lengths, arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'), iters=iters, lr=lr,
                                         weights=w, smooth=smooth, share_betas=share_betas, anchor=anchor)
            for h, s in enumerate(grp):
                parts[s].append({k: (getattr(r, k)[h] if len(grp) == 2 else getattr(r, k)).cpu().numpy() for k in ('para', 'verts', 'joints', 'joint_uv', 'mse_before',
                                                                                                                    'mse_after', 'status')})
                if st is not None:
                    parts[s][-1].update({n: (getattr(st, k)[h] if len(grp) == 2 else getattr(st, k)).cpu().numpy()
                                         for n, k in (('start', 'para'), ('start_status', 'status'), ('start_choice', 'choice'))})
                if lengths is not None:
                    d = parts[s][-1]
                    d['seq_status'] = (r.seq_status[h] if len(grp) == 2 else r.seq_status).cpu().numpy()
                    d['betas'] = np.full((len(lengths), 10), np.nan, np.float32)
                    f0 = 0
                    for i, length in enumerate(lengths):
                        live = np.nonzero((d['status'][f0:f0 + length] & MF.STATUS_PASSED_THROUGH) == 0)[0]
                        if live.size:
                            d['betas'][i] = d['para'][f0 + live[0], 51:61]
                        f0 += length
        for s in grp:
            out[s] = {k: np.concatenate([p[k] for p in parts[s]]) for k in parts[s][0]}
    return out


def layer_buffers(state, side):
    """what capsule_radii reads, from the checkpoint's th_* buffers of one side"""
    pre = 'init_regressor.mano_layer_%s.' % side
    return {'th_v_template': state[pre + 'th_v_template'].detach().cpu(), 'th_weights': state[pre + 'th_weights'].detach().cpu(),
            'th_J_regressor': state[pre + 'th_J_regressor'].detach().cpu(), 'side': side}


def fit_pair_targets(tables, targets, radii, offset=None, offset_conf=None, iters=200, lr=0.1, weights=None, bs=256, cam_scale=1.0, device='cuda',
                     start='neutral'):
    """both sides of read_targets' dict (the same N) fitted as pairs, one launch per batch -> (fit_targets' dict per side, {offset, collision,
    pair_status}) (numpy).  radii: {side: [20] array}; offset [N,3] / offset_conf [N]: the start (default 0) and, with w_off, the target; lr: fit_mano_pair's
    (a dict may hold 'offset'); weights: one dict over fit_mano's keys and w_col, w_off, w_off_init."""
    import torch

    from ..utils import mano_fit as MF
    if sorted(targets) != sorted(SIDES) or len({next(iter(targets[s].values())).shape[0] for s in SIDES}) != 1:
        raise ValueError('fit_mano: --pair needs targets for both sides with the same N')
    N = next(iter(targets['left'].values())).shape[0]
    if offset is not None and tuple(offset.shape) != (N, 3) or offset_conf is not None and (offset is None or tuple(offset_conf.shape) != (N,)):
        raise ValueError('fit_mano: offset must be [N,3] and offset_conf [N] (with offset)')
    rad = [torch.from_numpy(np.ascontiguousarray(np.asarray(radii[s], np.float32).reshape(20))).to(device) for s in SIDES]
    w = dict(weights or {})
    for k, t in (('w_verts', 'verts'), ('w_joints', 'joints'), ('w_uv', 'joint_uv')):
        if not any(t in targets[s] for s in SIDES):
            w[k] = 0.0
        else:
            w.setdefault(k, MF.DEFAULT_WEIGHTS[k])
    for k, d in MF.DEFAULT_PAIR_WEIGHTS.items():
        w.setdefault(k, d)
    parts, pparts = {s: [] for s in SIDES}, []
    for b0 in range(0, N, bs):
        b1 = min(b0 + bs, N)
        dev = lambda s, k: torch.from_numpy(np.ascontiguousarray(targets[s][k][b0:b1])).to(device) if k in targets[s] else None  # noqa: E731
        arg = lambda k: [dev(s, k) for s in SIDES]  # noqa: E731
        init = [dev(s, 'init') if 'init' in targets[s] else MF.neutral_para(b1 - b0, cam_scale, device) for s in SIDES]
        o0 = torch.zeros(b1 - b0, 3, device=device) if offset is None else torch.from_numpy(np.ascontiguousarray(offset[b0:b1], np.float32)).to(device)
        use_t = offset is not None and w['w_off'] > 0
        oc = None if offset_conf is None or not use_t else torch.from_numpy(np.ascontiguousarray(offset_conf[b0:b1], np.float32)).to(device)
        r = MF.fit_mano_pair([tables[s] for s in SIDES], init, o0, radii=rad, offset_target=o0 if use_t else None, offset_conf=oc, verts=arg('verts'),
                             joints=arg('joints'), joints_conf=arg('joints_conf'), joint_uv=arg('joint_uv'), uv_conf=arg('uv_conf'), iters=iters, lr=lr, weights=w,
                             start=start)
        for h, s in enumerate(SIDES):
            parts[s].append({k: getattr(r, k)[h].cpu().numpy() for k in ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after', 'status')})
        pparts.append({'offset': r.offset.cpu().numpy(), 'collision': r.collision.cpu().numpy(), 'pair_status': r.pair_status.cpu().numpy()})
    out = {s: {k: np.concatenate([p[k] for p in parts[s]]) for k in parts[s][0]} for s in SIDES}
    return out, {k: np.concatenate([p[k] for p in pparts]) for k in pparts[0]}


def main(argv=None):
    import argparse

    import torch

    from . import checkpoint_weights
    ap = argparse.ArgumentParser(description='fit MANO parameters (the 64-vector of pd_mano_para_*) to meshes, 3-D joints and 2-D keypoints on the GPU')
    ap.add_argument('--model', type=str, required=True, help='a DIR checkpoint: its MANO tables are used')
    ap.add_argument('--ema', action='store_true')
    ap.add_argument('--targets', type=str, required=True, help='T.npz: verts_/joints_/joints_conf_/joint_uv_/uv_conf_/init_<side>')
    ap.add_argument('--out', type=str, required=True)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--lr', type=float, default=0.1, help='the learning rate of every group (not tuned on real data)')
    for g in ('root', 'pca', 'betas', 'cam'):
        ap.add_argument('--lr_' + g, type=float, default=None, help='the learning rate of this group instead of --lr (0 freezes it)')
    ap.add_argument('--bs', type=int, default=256)
    ap.add_argument('--center', type=int, default=0, help='the joint 3-D targets are relative to (-1: none)')
    ap.add_argument('--cam_scale', type=float, default=1.0, help='the camera scale of the cold start')
    for k, d in (('w_verts', None), ('w_joints', None), ('w_uv', None), ('w_pca', 0.0), ('w_beta', 0.0), ('w_init', 0.0)):
        ap.add_argument('--' + k, type=float, default=d)
    ap.add_argument('--start', choices=('neutral', 'closed'), default='neutral', help='closed: root and camera of the start in closed form (dir_mano_fit_start)')
    ap.add_argument('--sequences', action='store_true', help='the hands are frames of the sequences seq_len [S] of T.npz: one fit over whole sequences')
    for k in ('w_t_root', 'w_t_pca', 'w_t_cam'):
        ap.add_argument('--' + k, type=float, default=1.0, help='--sequences: the temporal weight of this group (not tuned on real tracks)')
    ap.add_argument('--per_frame_shape', action='store_true', help='--sequences: betas per frame instead of one shape per (sequence, side)')
    ap.add_argument('--pair', action='store_true', help='row n of both sides is one person: fit the two hands together with their offset and a collision term')
    ap.add_argument('--w_col', type=float, default=None, help='--pair: the weight of the capsule collision term (not tuned)')
    ap.add_argument('--w_offset', type=float, default=0.0, help="--pair: the weight of the pull to the targets' offset")
    ap.add_argument('--w_offset_init', type=float, default=0.0, help='--pair: the weight of the pull to the starting offset')
    ap.add_argument('--lr_offset', type=float, default=None, help='--pair: the learning rate of the offset instead of --lr (0 freezes it)')
    ap.add_argument('--radii', type=str, default='auto', help="--pair: 'auto' (capsule_radii of the checkpoint's tables) or an .npz with radii_left, radii_right [20]")
    opt = ap.parse_args(argv)
    if opt.bs < 1 or opt.iters < 0 or not -1 <= opt.center < 21:
        ap.error('--bs must be at least 1, --iters at least 0 and --center in -1 .. 20')
    if opt.pair and (opt.sequences or opt.center < 0):
        ap.error('--pair needs --center >= 0 (the offset joins the two centre joints) and does not combine with --sequences')
    seq_len = smooth = offset = offset_conf = None
    with np.load(opt.targets) as f:
        targets = read_targets(f)
        if opt.pair:
            offset = np.asarray(f['offset'], np.float32) if 'offset' in f else None
            offset_conf = np.asarray(f['offset_conf'], np.float32) if 'offset_conf' in f else None
        if opt.sequences:
            if 'seq_len' not in f:
                ap.error('--sequences needs seq_len [S] in the targets')
            seq_len = np.asarray(f['seq_len']).astype(np.int64).reshape(-1)
            smooth = {'root': opt.w_t_root, 'pca': opt.w_t_pca, 'cam': opt.w_t_cam}
            if min(smooth.values()) < 0:
                ap.error('--w_t_root, --w_t_pca and --w_t_cam must be >= 0')
    state = checkpoint_weights(torch.load(opt.model, map_location='cpu', weights_only=False), opt.ema, opt.model)
    tables, keep = tables_from_checkpoint(state, opt.center)
    lr = {g: (getattr(opt, 'lr_' + g) if getattr(opt, 'lr_' + g) is not None else opt.lr) for g in ('root', 'pca', 'betas', 'cam')}
    weights = {k: getattr(opt, k) for k in ('w_verts', 'w_joints', 'w_uv', 'w_pca', 'w_beta', 'w_init') if getattr(opt, k) is not None}
    extra = {}
    if opt.pair:
        from ..utils import mano_fit as MF
        if opt.radii == 'auto':
            radii = {s: MF.capsule_radii(layer_buffers(state, s)).numpy() for s in SIDES}
        else:
            with np.load(opt.radii) as f:
                radii = {s: np.asarray(f['radii_' + s], np.float32) for s in SIDES}
        lr['offset'] = opt.lr if opt.lr_offset is None else opt.lr_offset
        weights.update(w_off=opt.w_offset, w_off_init=opt.w_offset_init, **({} if opt.w_col is None else {'w_col': opt.w_col}))
    t0 = time.perf_counter()
    if opt.pair:
        res, extra = fit_pair_targets(tables, targets, radii, offset, offset_conf, opt.iters, lr, weights, opt.bs, opt.cam_scale, start=opt.start)
    else:
        res = fit_targets(tables, targets, opt.iters, lr, weights, opt.bs, opt.cam_scale, start=opt.start, seq_len=seq_len, smooth=smooth,
                          share_betas=not opt.per_frame_shape)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    np.savez(opt.out, **{'%s_%s' % (k, s): v for s, d in res.items() for k, v in d.items()}, **extra)
    n = sum(d['para'].shape[0] for d in res.values())
    for s, d in res.items():
        with np.errstate(invalid='ignore'):
            print('%s: %d hands, mean squared residual (verts, joints, joint_uv) %s -> %s, %d with a status' % (
                s, d['para'].shape[0], d['mse_before'].mean(0).tolist(), d['mse_after'].mean(0).tolist(), int((d['status'] != 0).sum())))
    if opt.pair:
        c = extra['collision']
        print('pairs: largest capsule overlap %.2f -> %.2f mm, %d with a pair status' % (c[:, 1].max() * 1e3, c[:, 3].max() * 1e3, int((extra['pair_status'] != 0).sum())))
    print('%d hands in %.2f s' % (n, sec))
    return n


if __name__ == '__main__':
    main()
