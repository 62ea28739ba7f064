"""MANO parameters from meshes, 3-D joints and 2-D keypoints: dir_mano_fit (csrc/mano_fit.hip) behind a small Python surface.  The rule -- a
residual over one hand's 64-vector (6D root, 45 PCA coefficients, 10 betas, 3 camera scalars) walked down by Adam inside ONE launch -- is
written out in include/dir_hip.h ("MANO fitting"); nothing here does arithmetic on the GPU but that launch.

    res = fit_mano(layer, neutral_para(B), verts=meshes, iters=200, lr=0.1, weights={'w_verts': 1e4})
    res.para [B,64], res.verts / joints / joint_uv at the fitted parameters, res.mse_before / mse_after [B,3], res.status [B], res.state

`layer_or_tables`: a dir_amd.manopth.manolayer.ManoLayer (its own center_idx), a _capi.ManoTables, or a list of two of either for a pair of
hands; with a pair every other tensor argument is a list of two (an entry may be None).  The defaults (lr, weights, iteration counts) are NOT
tuned on real MANO tables or real keypoints.

    st = start_mano(layer, neutral_para(B), verts=meshes)         # dir_mano_fit_start: root and camera in closed form, one launch
    st.para [B,64], st.status [B], st.choice [B], st.info [B,4]
    res = fit_mano(layer, neutral_para(B), verts=meshes, start='closed')      # the two launches, the fit anchored at the started parameters

The start (include/dir_hip.h, "MANO fitting: closed-form start") turns the root onto 3-D targets by a rigid alignment of the points that are
rigid under it, or, with 2-D targets alone, picks one of the cube's 24 rotations, and fits the camera by least squares: an arbitrary rotation
is no longer out of Adam's reach, and cam_scale need not be guessed.

    res = fit_mano_sequence(layer, neutral_para(N), seq_lengths, joints=tracks, joints_conf=conf, smooth={'root': 1, 'pca': 1, 'cam': 1})
    res.para [N,64] (one shape per sequence in every frame's 51:61), ..., res.seq_status [S]

Whole sequences (include/dir_hip.h, "MANO fitting: sequences"; csrc/mano_fit_seq.hip): the N frames of S sequences laid end to end are ONE optimisation --
one shape per (sequence, hand), a pose and a camera per frame, neighbouring frames coupled in time -- so the betas do not change from frame to frame and a
frame without keypoints is filled from its neighbours.  One launch per iteration (two with the shared shape), all enqueued by one library call.

    res = fit_mano_pair([left, right], [init_l, init_r], offset0, radii=[capsule_radii(left), capsule_radii(right)], joints=[jl, jr], weights={'w_joints': 1e4, 'w_col': 1e4})
    res.para / verts / ... lists of two as fit_mano's pair form, res.offset [B,3], res.collision [B,4], res.pair_status [B]

Two hands together (include/dir_hip.h, "MANO fitting: two hands together"; csrc/mano_fit_pair.hip): the two hands of a pair and the offset between their centre
joints are ONE optimisation, with a capsule per bone that keeps the hands from passing through each other.  One launch, one 512-thread workgroup per pair.
"""
import collections

import torch

from .. import _capi
from .. import functional as F

GROUPS = F.MANO_FIT_GROUPS                                   # root 0:6, pca 6:51, betas 51:61, cam 61:64
DEFAULT_WEIGHTS = {'w_verts': 1e4, 'w_joints': 1e4, 'w_uv': 1.0, 'w_pca': 0.0, 'w_beta': 0.0, 'w_init': 0.0}
STATUS_REFLECTION, STATUS_PASSED_THROUGH, STATUS_NONFINITE_STEP = 1, 2, 4
STATUS_ROOT_KEPT, STATUS_CAM_KEPT = 8, 16                    # start_mano only: a step that ran left p0's root / camera in place

FitResult = collections.namedtuple('FitResult', 'para verts joints joint_uv mse_before mse_after status state')
StartResult = collections.namedtuple('StartResult', 'para status choice info')


def neutral_para(B, cam_scale=1.0, device='cuda'):
    """the cold start [B,64]: root 6D (1,0,0, 0,1,0), zero PCA coefficients and betas, cam (cam_scale, 0, 0)"""
    p = torch.zeros(B, 64, device=device)
    p[:, 0] = 1.0
    p[:, 4] = 1.0
    p[:, 61] = float(cam_scale)
    return p


def new_state(B, device='cuda'):
    """a fresh Adam state [B, 132]: m | v | b1^t | b2^t | t | 0 -- all zeros"""
    return torch.zeros(B, _capi.MANO_FIT_STATE, device=device)


def _lr4(lr):
    if isinstance(lr, dict):
        if set(lr) - set(GROUPS):
            raise ValueError('fit_mano: lr groups are %s, got %s' % (GROUPS, sorted(lr)))
        return [float(lr.get(g, 0.0)) for g in GROUPS]
    return [float(lr)] * 4


def _tables(x):
    return x if isinstance(x, _capi.ManoTables) else x.c_tables(x.center_idx)


def _term_weights(weights, verts, joints, joint_uv):
    if weights is None:
        return {k: (DEFAULT_WEIGHTS[k] if t is not None else 0.0) for k, t in (('w_verts', verts), ('w_joints', joints), ('w_uv', joint_uv))}
    return weights


_Hands = collections.namedtuple('_Hands', 'pair hands ls opt tabs p0 B dev')


def _hands(who, layer_or_tables, init):
    """What start_mano, fit_mano and fit_mano_sequence make of their first two arguments: pair (lists of two were given), hands, ls (an argument as
    the list per hand), opt (the same for an optional tensor argument, as contiguous float32), the tables, the starts p0, their rows B and device"""
    pair = isinstance(layer_or_tables, (list, tuple))
    hands = 2 if pair else 1
    ls = lambda x: list(x) if pair else [x]  # noqa: E731
    opt = lambda x: None if x is None else [None if t is None else _capi.f32c(t) for t in ls(x)]  # noqa: E731
    tabs = [_tables(x) for x in ls(layer_or_tables)]
    p0 = [_capi.f32c(t) for t in ls(init)]
    if len(tabs) != hands or len(p0) != hands:
        raise ValueError('%s: a pair takes lists of two' % who)
    return _Hands(pair, hands, ls, opt, tabs, p0, p0[0].shape[0], p0[0].device)


def _closed_start(layer_or_tables, init, anchor, verts, joints, joints_conf, joint_uv, uv_conf, weights):
    """start='closed': start_mano's parameters are the fit's start, and its anchor where none is given.  -> init, anchor"""
    init = start_mano(layer_or_tables, init, verts, joints, joints_conf, joint_uv, uv_conf, weights).para
    return init, (init if anchor is None else anchor)


def _fit_results(res, p0, st, dev):
    """functional's per-hand dicts as one FitResult per hand.  res None: the empty batch, nothing was launched.  st: None, or the state per hand"""
    state = lambda h: None if st is None else st[h]  # noqa: E731
    if res is None:
        e = lambda *s: torch.empty((0,) + s, device=dev)  # noqa: E731
        return [FitResult(p.clone(), e(778, 3), e(21, 3), e(21, 2), e(3), e(3), torch.empty(0, dtype=torch.int32, device=dev), state(h)) for h, p in enumerate(p0)]
    return [FitResult(r['para'], r.get('verts'), r.get('joints'), r.get('joint_uv'), r['mse'][:, :3], r['mse'][:, 3:], r['status'], state(h))
            for h, r in enumerate(res)]


def start_mano(layer_or_tables, init, verts=None, joints=None, joints_conf=None, joint_uv=None, uv_conf=None, weights=None, root=True, cam=True, search=True):
    """One launch of dir_mano_fit_start: init [B,64] (not written) with its root and camera moved in closed form towards the targets (fit_mano's, each
    optional).  weights: fit_mano's dict (only w_verts and w_joints are read, as the two 3-D terms' weights against one another).  root / cam: the
    step may write that group; search: with 2-D targets alone, try the cube's 24 rotations.  -> StartResult(para [B,64], status [B] (bit 0 reflection,
    bit 1 non-finite input: both passed through; 8 root kept, 16 camera kept), choice [B] (the rotation the search wrote, else -1), info [B,4] (3-D
    energy before, after; 2-D residual before, after)); lists of two per field for a pair."""
    pair, _, _, opt, tabs, p0, B, dev = _hands('start_mano', layer_or_tables, init)
    w = _term_weights(weights, verts, joints, joint_uv)
    if B == 0:
        rs = [StartResult(p.clone(), torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 4, device=dev))
              for p in p0]
    else:
        res = F.mano_fit_start(tabs, p0, opt(verts), opt(joints), opt(joints_conf), opt(joint_uv), opt(uv_conf), w.get('w_verts', 0.0), w.get('w_joints', 0.0),
                               root, cam, search)
        rs = [StartResult(r['para'], r['status'], r['choice'], r['info']) for r in res]
    return StartResult(*[list(f) for f in zip(*rs)]) if pair else rs[0]


def fit_mano(layer_or_tables, init, verts=None, joints=None, joints_conf=None, joint_uv=None, uv_conf=None, iters=200, lr=0.1, weights=None,
             state=None, outputs=True, anchor=None, betas=(0.9, 0.999), eps=1e-8, start=None):
    """One launch of dir_mano_fit.  init [B,64] float32 on the GPU (not written); targets verts [B,778,3], joints [B,21,3] with joints_conf [B,21],
    joint_uv [B,21,2] with uv_conf [B,21] (each optional; a confidence of 0 selects the entry out, which may then hold NaN).  lr: a float, or a
    dict per group of GROUPS (a missing group is frozen).  weights: dict over w_verts, w_joints, w_uv, w_pca, w_beta, w_init; None: DEFAULT_WEIGHTS
    for the terms whose targets are given.  state: True for a fresh Adam state, or the `state` of an earlier result to go on from it (updated
    in place; pass the same `anchor` -- None: init -- so that a + b iterations equal the two runs bit for bit).  outputs=False: no verts /
    joints / joint_uv.  start: None (every launch and byte as without it), or 'closed': start_mano(init, the same targets and weights) runs first and
    the fit starts from its parameters, which are also the anchor where none is given.  -> FitResult (lists of two per field for a pair)."""
    if start not in (None, 'closed'):
        raise ValueError("fit_mano: start is None or 'closed', got %r" % (start,))
    if start == 'closed':
        init, anchor = _closed_start(layer_or_tables, init, anchor, verts, joints, joints_conf, joint_uv, uv_conf, weights)
    pair, hands, ls, opt, tabs, p0, B, dev = _hands('fit_mano', layer_or_tables, init)
    weights = _term_weights(weights, verts, joints, joint_uv)
    if state is True:
        state = [new_state(B, dev) for _ in range(hands)]
        state = state if pair else state[0]
    st = None if state is None else ls(state)
    res = None if B == 0 else F.mano_fit(tabs, p0, opt(verts), opt(joints), opt(joints_conf), opt(joint_uv), opt(uv_conf), iters, _lr4(lr), weights, betas, eps,
                                         opt(anchor), st, outputs)
    rs = _fit_results(res, p0, st, dev)
    return FitResult(*[list(f) for f in zip(*rs)]) if pair else rs[0]


# ---- whole sequences: dir_mano_fit_sequence (csrc/mano_fit_seq.hip; include/dir_hip.h, "MANO fitting: sequences")
DEFAULT_SMOOTH = {'root': 1.0, 'pca': 1.0, 'cam': 1.0}       # w_t_root, w_t_pca, w_t_cam: NOT tuned on real tracks
STATUS_NO_DATA = 8                                           # fit_mano_sequence only: a non-finite target in use, the frame's data terms were dropped
SEQ_STATUS_EMPTY, SEQ_STATUS_SHAPE_FROZEN = 2, 4
SeqFitResult = collections.namedtuple('SeqFitResult', FitResult._fields + ('seq_status',))
SeqState = collections.namedtuple('SeqState', 'frames seq')  # the frames' Adam state [N,132] and the shared shapes' [S,24] (lists of two for a pair)


def new_seq_state(N, S, hands=1, device='cuda'):
    """a fresh state for fit_mano_sequence: all zeros"""
    fr = [torch.zeros(N, _capi.MANO_FIT_STATE, device=device) for _ in range(hands)]
    sq = [torch.zeros(S, _capi.MANO_FIT_SEQ_STATE, device=device) for _ in range(hands)]
    return SeqState(fr, sq) if hands == 2 else SeqState(fr[0], sq[0])


def fit_mano_sequence(layer_or_tables, init, seq_lengths, verts=None, joints=None, joints_conf=None, joint_uv=None, uv_conf=None, iters=200, lr=0.1,
                      weights=None, smooth=None, share_betas=True, state=None, outputs=True, anchor=None, betas=(0.9, 0.999), eps=1e-8, start='neutral',
                      work=None):
    """dir_mano_fit_sequence: one optimisation over whole sequences.  init [N,64] and the targets as fit_mano's, with the N frames of the sequences laid
    end to end; seq_lengths: their lengths (ints on the host, each >= 1, summing to N).  One shape per (sequence, hand) with share_betas (else one per
    frame), a pose and a camera per frame, and the temporal term `smooth` = {'root':, 'pca':, 'cam':} (None: DEFAULT_SMOOTH; a missing key is 0) between
    neighbouring frames.  A frame whose confidences are all 0 is filled from its neighbours; a frame with a non-finite init passes through and splits its
    sequence.  state: True for a fresh one, or the SeqState of an earlier result (updated in place; pass the same `anchor`).  start: 'neutral', or
    'closed': start_mano(init, the same targets and weights) runs per frame first, and its parameters are the anchor where none is given.  work: a uint8
    workspace of functional.mano_fit_sequence_workspace_bytes to reuse.  -> SeqFitResult: fit_mano's fields over the N frames (para holds the sequence's
    betas in every frame) + seq_status [S] (2: no usable frame, 4: the shared shape was frozen); lists of two per field for a pair."""
    if start not in ('neutral', 'closed'):
        raise ValueError("fit_mano_sequence: start is 'neutral' or 'closed', got %r" % (start,))
    if start == 'closed':
        init, anchor = _closed_start(layer_or_tables, init, anchor, verts, joints, joints_conf, joint_uv, uv_conf, weights)
    pair, hands, ls, opt, tabs, p0, N, dev = _hands('fit_mano_sequence', layer_or_tables, init)
    lengths = [int(n) for n in seq_lengths]
    if any(n < 1 for n in lengths) or sum(lengths) != N:
        raise ValueError('fit_mano_sequence: seq_lengths must be >= 1 and sum to the %d frames, got %s' % (N, lengths[:8]))
    S = len(lengths)
    smooth = DEFAULT_SMOOTH if smooth is None else smooth
    if set(smooth) - set(DEFAULT_SMOOTH):
        raise ValueError('fit_mano_sequence: smooth keys are %s, got %s' % (sorted(DEFAULT_SMOOTH), sorted(smooth)))
    weights = _term_weights(weights, verts, joints, joint_uv)
    if state is True:
        state = new_seq_state(N, S, hands, dev)
    fr, sq = (None, None) if state is None else (ls(state.frames), ls(state.seq))
    starts = [0]
    for n in lengths:
        starts.append(starts[-1] + n)
    if N == 0:                           # (every hand's state field is the state as given)
        rs = [SeqFitResult(*f, torch.empty(0, dtype=torch.int32, device=dev)) for f in _fit_results(None, p0, None if state is None else [state] * hands, dev)]
        return SeqFitResult(*[list(f) for f in zip(*rs)]) if pair else rs[0]
    res, seq_status = F.mano_fit_sequence(tabs, p0, torch.tensor(starts, dtype=torch.int32).to(dev), opt(verts), opt(joints), opt(joints_conf), opt(joint_uv),
                                          opt(uv_conf), iters, _lr4(lr), weights, [float(smooth.get(k, 0.0)) for k in ('root', 'pca', 'cam')], share_betas, betas,
                                          eps, opt(anchor), fr, sq, outputs, work=work, seq_start_host=starts)
    st = None if state is None else [SeqState(fr[h], sq[h]) for h in range(hands)]
    rs = [SeqFitResult(*f, seq_status[h]) for h, f in enumerate(_fit_results(res, p0, st, dev))]
    if not pair:
        return rs[0]
    out = SeqFitResult(*[list(f) for f in zip(*rs)])
    return out._replace(state=state)


# ---- two hands together: dir_mano_fit_pair (csrc/mano_fit_pair.hip; include/dir_hip.h, "MANO fitting: two hands together")
DEFAULT_PAIR_WEIGHTS = {'w_col': 1e4, 'w_off': 0.0, 'w_off_init': 0.0}      # NOT tuned: this tree has no real MANO tables
PAIR_STATUS_HAND_PASSED, PAIR_STATUS_OFFSET_PASSED, PAIR_STATUS_OFFSET_FROZEN, PAIR_STATUS_NO_DIRECTION = 1, 2, 4, 8
BONE_PARENT = (0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19)           # bone k joins joints BONE_PARENT[k] and k + 1
_REORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)       # output joint -> chain joint (0..15) or fingertip (16..20)
_TIPS = {'right': (745, 317, 444, 556, 673), 'left': (745, 317, 445, 556, 673)}
PairFitResult = collections.namedtuple('PairFitResult', FitResult._fields + ('offset', 'collision', 'pair_status', 'offset_state'))


def new_offset_state(B, device='cuda'):
    """a fresh Adam state of the offset [B, 12]: m | v | b1^t | b2^t | t | 0 0 0 -- all zeros"""
    return torch.zeros(B, _capi.MANO_FIT_PAIR_STATE, device=device)


def capsule_radii(layer_or_tables, q=0.5):
    """One radius per bone [20] (float32, on the tables' device) for fit_mano_pair's capsules, from the template pose: bone k joins output joints
    BONE_PARENT[k] and k + 1; its radius is the q-quantile of the distances to that segment over the vertices whose largest skinning weight belongs to the
    bone's parent joint (the five fingertip bones have a fingertip as their child: their vertices are the last chain joint's, the child's side).  A bone
    without such a vertex gets 0.  Plain torch, done once.  layer_or_tables: a ManoLayer, or a mapping with th_v_template [778,3], th_weights [778,16],
    th_J_regressor [16,778] and 'side' (a _capi.ManoTables holds bare pointers and cannot be read here).  UNTUNED: q, like every default weight of
    fit_mano_pair, has not been set on real MANO tables -- this tree has none."""
    get = (lambda k: layer_or_tables[k]) if isinstance(layer_or_tables, dict) else (lambda k: getattr(layer_or_tables, k))
    v = get('th_v_template').reshape(778, 3).double()
    w = get('th_weights').reshape(778, 16).double()
    jr = get('th_J_regressor').reshape(16, 778).double()
    side = get('side')
    src = torch.cat([jr @ v, v[list(_TIPS[side])]], 0)[list(_REORDER)]                 # the 21 output joints at the template pose
    owner = w.argmax(1)                                                               # chain joint of each vertex
    out = torch.zeros(20, dtype=torch.float64, device=v.device)
    for k in range(20):
        pa = BONE_PARENT[k]
        chain = _REORDER[pa]                                                          # always < 16: no bone starts at a fingertip
        pts = v[owner == chain]
        if pts.shape[0] == 0:
            continue
        a, b = src[pa], src[k + 1]
        ab = b - a
        t = ((pts - a) @ ab / (ab @ ab).clamp(min=1e-30)).clamp(0, 1)
        out[k] = torch.quantile((pts - (a + t[:, None] * ab)).norm(dim=1), float(q))
    return out.float().contiguous()


def fit_mano_pair(layers_or_tables, init, offset0, *, radii=None, offset_target=None, offset_conf=None, offset_anchor=None, verts=None, joints=None,
                  joints_conf=None, joint_uv=None, uv_conf=None, iters=200, lr=0.1, weights=None, state=None, anchor=None, start='neutral', outputs=True,
                  betas=(0.9, 0.999), eps=1e-8):
    """One launch of dir_mano_fit_pair: both hands of B pairs fitted together with the offset o [B,3] (right centre joint minus left, metres; 0.15 x the
    network's pd_offset) and a capsule-per-bone collision term between the hands.  layers_or_tables, init and every per-hand target: lists of two (left
    slot, right slot), as fit_mano's pair form.  radii: two [20] tensors (None: capsule_radii of the two layers, q = 0.5).  lr: a float, or a dict over
    GROUPS + ('offset',) (a missing group is frozen).  weights: one dict over fit_mano's keys and w_col, w_off, w_off_init (None: DEFAULT_WEIGHTS for the
    terms whose targets are given, and DEFAULT_PAIR_WEIGHTS).  state: True for fresh ones, or (the list of two hand states, the offset state) of an earlier
    result.  start: 'neutral', or 'closed' (start_mano per hand first, as fit_mano).  -> PairFitResult: fit_mano's pair result + offset [B,3], collision
    [B,4] (mean squared overlap and largest overlap in metres at the start, then at the end) and pair_status [B].  Every default (radii quantile, weights, rates) is
    UNTUNED: this tree has no real MANO tables."""
    if start not in ('neutral', 'closed'):
        raise ValueError("fit_mano_pair: start is 'neutral' or 'closed', got %r" % (start,))
    if len(layers_or_tables) != 2 or len(init) != 2:
        raise ValueError('fit_mano_pair: takes lists of two')
    term_w = None if weights is None else {k: v for k, v in weights.items() if k in F.MANO_FIT_WEIGHTS}
    pair_w = dict(DEFAULT_PAIR_WEIGHTS) if weights is None else {k: v for k, v in weights.items() if k in F.MANO_FIT_PAIR_WEIGHTS}
    if weights is not None and set(weights) - set(F.MANO_FIT_WEIGHTS) - set(F.MANO_FIT_PAIR_WEIGHTS):
        raise ValueError('fit_mano_pair: unknown weights %s' % sorted(set(weights) - set(F.MANO_FIT_WEIGHTS) - set(F.MANO_FIT_PAIR_WEIGHTS)))
    if start == 'closed':
        init, anchor = _closed_start(list(layers_or_tables), list(init), anchor, verts, joints, joints_conf, joint_uv, uv_conf, term_w)
    opt = lambda x: None if x is None else [None if t is None else _capi.f32c(t) for t in x]  # noqa: E731
    one = lambda t: None if t is None else _capi.f32c(t)  # noqa: E731
    tabs = [_tables(x) for x in layers_or_tables]
    p0 = [_capi.f32c(t) for t in init]
    B, dev = p0[0].shape[0], p0[0].device
    if radii is None:
        radii = [capsule_radii(x).to(dev) for x in layers_or_tables]
    if isinstance(lr, dict):
        if set(lr) - set(GROUPS) - {'offset'}:
            raise ValueError("fit_mano_pair: lr groups are %s and 'offset', got %s" % (GROUPS, sorted(lr)))
        lr4, lr_o = [float(lr.get(g, 0.0)) for g in GROUPS], float(lr.get('offset', 0.0))
    else:
        lr4, lr_o = [float(lr)] * 4, float(lr)
    term_w = _term_weights(term_w, verts, joints, joint_uv)
    if state is True:
        state = ([new_state(B, dev), new_state(B, dev)], new_offset_state(B, dev))
    st, ost = (None, None) if state is None else (list(state[0]), state[1])
    o0 = _capi.f32c(offset0)
    if B == 0:
        pr = {'offset': o0.clone(), 'col': torch.empty(0, 4, device=dev), 'pair_status': torch.empty(0, dtype=torch.int32, device=dev)}
        res = None
    else:
        res, pr = F.mano_fit_pair(tabs, p0, o0, [_capi.f32c(r) for r in radii], opt(verts), opt(joints), opt(joints_conf), opt(joint_uv), opt(uv_conf), iters, lr4,
                                  lr_o, term_w, pair_w, one(offset_target), one(offset_conf), one(offset_anchor), betas, eps, opt(anchor), st, ost, outputs)
    return PairFitResult(*[list(f) for f in zip(*_fit_results(res, p0, st, dev))], pr['offset'], pr['col'], pr['pair_status'], ost)
