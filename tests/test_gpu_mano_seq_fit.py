"""GPU: dir_mano_fit_sequence (csrc/mano_fit_seq.hip) -- MANO fitted to whole sequences: one shape per (sequence, hand), a pose and a camera per
frame, neighbouring frames coupled in time -- against the float64 restatement of its rule (tests/helpers/mano_seq_fit_ref.py), against dir_mano_fit
where the two rules coincide, and the Python surface on top of it (utils/mano_fit.py fit_mano_sequence, apps/fit_mano.py --sequences).

Gates: |kernel - float64 restatement| <= 4 x the largest |float32 restatement - float64 restatement| that tests/test_mano_seq_fit_ref.py measured on
the CPU for that configuration, iteration count and output (mano_seq_fit_ref.GATES); nothing here is measured on the kernel.  Every figure is printed
before it is asserted.  The shapes beyond the canonical case (T = 1, 2, 3, the lengths around the shape reduction's boundaries) run 2 iterations and
are held to the canonical case's 2-iteration gates.

Measured on the MI355X (information, not a bound): the kernels used at most 0.59 of a gate over both configurations x 1, 2, 10, 50 iterations x both hands
and the eleven shapes; every bit equality held."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import mano_fit_ref as R  # noqa: E402
import mano_gpu_run as G  # noqa: E402
import mano_seq_fit_ref as Q  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd import functional as F  # noqa: E402
from dir_amd.utils import mano_fit as MF  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after', 'status')
WAVE, LANES = 64, _capi.MANO_FIT_SEQ_LANES          # the shape reduction: lane l of LANES adds frames l, l + LANES, ...; waves of WAVE lanes; 4 waves in order
_REF, _PROB = {}, {}


def canonical(side):
    if side not in _PROB:
        _PROB[side] = Q.canonical(side)[0]
    return _PROB[side]


def ref64(side, iters, share):
    """the float64 restatement on the canonical case: computed once, shared, not to be written to"""
    key = (side, iters, share)
    if key not in _REF:
        _REF[key] = Q.fit_sequence(canonical(side), Q.LENGTHS, iters, torch.float64, share=share)
    return _REF[key]


def tables(prob):
    return G.packed(R.KIND, prob.side, prob.center, prob.root_palm)


def dev(a, rows=None):
    if a is None:
        return None
    a = np.asarray(a, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).cuda()


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def rows_of(prob, rows):
    return prob._replace(**{k: (None if getattr(prob, k) is None else getattr(prob, k)[rows]) for k in ('init', 'joints', 'joints_conf')})


def run(probs, lengths, iters, smooth=Q.SMOOTH, share=True, state=None, anchor=None, init=None, **kw):
    """fit_mano_sequence on one Problem (one hand) or a list of two (a pair) -> SeqFitResult of device tensors"""
    pair = not isinstance(probs, R.Problem)
    ps = list(probs) if pair else [probs]
    arg = lambda k: [dev(getattr(p, k)) for p in ps] if pair else dev(getattr(ps[0], k))  # noqa: E731
    p0 = arg('init') if init is None else init
    return MF.fit_mano_sequence([tables(p) for p in ps] if pair else tables(ps[0]), p0, lengths, joints=arg('joints'), joints_conf=arg('joints_conf'), iters=iters,
                                lr=dict(zip(MF.GROUPS, ps[0].lr)), weights=ps[0].weights, smooth=dict(zip(('root', 'pca', 'cam'), smooth)), share_betas=share,
                                state=state, anchor=anchor, **kw)


def hand(res, h):
    return type(res)(*[None if f is None else f[h] for f in res])


def same(a, b, fields=FIELDS, ra=slice(None), rb=slice(None)):
    return all(torch.equal(bits(getattr(a, k))[ra], bits(getattr(b, k))[rb]) for k in fields)


def check_against(got, ref, gates, what, worst):
    """every output of the frames inside its gate, the shape too; the status words exactly; an inert frame: p0's bits back"""
    assert got.status.tolist() == ref['status'].tolist() and got.seq_status.tolist() == ref['seq_status'].tolist(), (what, got.status.tolist(), got.seq_status.tolist())
    live = torch.isfinite(ref['para']).all(1)
    for k in R.OUTPUTS:
        d = float((getattr(got, k).double().cpu() - ref[k])[live].abs().max())
        worst[what + (k,)] = (d, Q.MARGIN * gates[k])
    first = [int(torch.nonzero(live[s0:s1])[0]) + s0 for s0, s1 in zip(ref_starts(ref), ref_starts(ref)[1:]) if bool(live[s0:s1].any())]
    shape = got.para[first, 51:61].double().cpu()
    worst[what + ('shape',)] = (float((shape - ref['shape'][[bool(live[s0:s1].any()) for s0, s1 in zip(ref_starts(ref), ref_starts(ref)[1:])]]).abs().max()),
                                Q.MARGIN * gates['shape'])


def ref_starts(ref):
    return ref['_starts']


def with_starts(ref, lengths):
    return dict(ref, _starts=[int(x) for x in Q.starts_of(lengths)])


@pytest.mark.parametrize('config', ['shared', 'per_frame'])
def test_canonical_case_against_the_float64_restatement(config):
    """iters 1, 2, 10, 50, both hands in one call (9 frames in sequences of 1, 3, 5 x 2 hands): V, J, U at the fitted p, mse_after, p itself and the shapes
    inside 4 x the CPU-recorded float32-against-float64 differences; status and seq_status exactly"""
    share = Q.CONFIGS[config]
    pl, pr = canonical('left'), canonical('right')
    worst = {}
    for it in Q.ITERS:
        pair = run([pl, pr], Q.LENGTHS, it, share=share)
        torch.cuda.synchronize()
        for h, (side, prob) in enumerate((('left', pl), ('right', pr))):
            got, ref = hand(pair, h), with_starts(ref64(side, it, share), Q.LENGTHS)
            check_against(got, ref, Q.GATES[config][it], (it, side), worst)
            assert torch.equal(bits(got.para[Q.INERT]), bits(dev(prob.init)[Q.INERT])) and float(got.verts[Q.INERT].abs().max()) == 0.0
            if share:
                for s0, s1 in ((1, 4), (4, 9)):
                    rows = [n for n in range(s0, s1) if n != Q.INERT]
                    assert all(torch.equal(bits(got.para[n, 51:61]), bits(got.para[rows[0], 51:61])) for n in rows)
    for key, (d, g) in sorted(worst.items()):
        print(config, key, 'difference %.3g gate %.3g (%.2f of it)' % (d, g, d / g))
    for key, (d, g) in worst.items():
        assert d <= g, (config, key, d, g)


def forward_bits(prob, para):
    B = para.shape[0]
    v, j, u = torch.empty(B, 778, 3, device='cuda'), torch.empty(B, 21, 3, device='cuda'), torch.empty(B, 21, 2, device='cuda')
    base = para.data_ptr()
    _capi.check(_capi.lib().dir_mano_forward(tables(prob), C.c_void_p(base), 64, C.c_void_p(base + 51 * 4), 64, C.c_void_p(base + 61 * 4), 64, _capi.ptr(v), _capi.ptr(j),
                                             _capi.ptr(u), None, None, B, _capi.stream_ptr()), 'dir_mano_forward')
    return v, j, u


def test_zero_temporal_weights_and_a_shape_per_frame_are_dir_mano_fit_bit_for_bit():
    """(a) para, verts, joints, joint_uv, mse, status and the Adam state equal dir_mano_fit on the same rows for iters 0, 1 and 10 (the inert frame is
    dir_mano_fit's pass-through row); at iters = 0 the outputs are dir_mano_forward's"""
    pl, pr = canonical('left'), canonical('right')
    N = sum(Q.LENGTHS)
    arg = lambda k: [dev(getattr(p, k)) for p in (pl, pr)]  # noqa: E731
    for iters in (0, 1, 10):
        st_seq = MF.new_seq_state(N, len(Q.LENGTHS), 2)
        seq = run([pl, pr], Q.LENGTHS, iters, smooth=(0.0, 0.0, 0.0), share=False, state=st_seq)
        st_fit = [MF.new_state(N), MF.new_state(N)]
        fit = MF.fit_mano([tables(pl), tables(pr)], arg('init'), joints=arg('joints'), joints_conf=arg('joints_conf'), iters=iters, lr=dict(zip(MF.GROUPS, pl.lr)),
                          weights=pl.weights, state=st_fit)
        torch.cuda.synchronize()
        for h, prob in enumerate((pl, pr)):
            assert same(hand(seq, h), hand(fit, h)), (iters, h, [k for k in FIELDS if not torch.equal(bits(getattr(seq, k)[h]), bits(getattr(fit, k)[h]))])
            assert torch.equal(bits(st_seq.frames[h]), bits(st_fit[h])) and seq.status[h].tolist() == [0] * 6 + [2] + [0] * 2
            assert st_seq.frames[h][:, 130].view(torch.int32).tolist() == [iters] * 6 + [0] + [iters] * 2
            assert float(st_seq.seq[h].abs().max()) == 0.0                # no shared shape: its state is untouched
            if iters == 0:
                live = [n for n in range(N) if n != Q.INERT]
                p0 = dev(prob.init)
                for got, want in zip((seq.verts[h], seq.joints[h], seq.joint_uv[h]), forward_bits(prob, p0[live])):
                    assert torch.equal(bits(got[live]), bits(want))
                assert torch.equal(bits(seq.para[h]), bits(p0))


def permuted(prob, order, lengths=Q.LENGTHS):
    """the canonical sequences laid out in another order -> (Problem, lengths, the first row of each original sequence in the new layout)"""
    st = Q.starts_of(lengths)
    rows = np.concatenate([np.arange(st[s], st[s + 1]) for s in order])
    at, n = {}, 0
    for s in order:
        at[s] = n
        n += lengths[s]
    return rows_of(prob, rows), [lengths[s] for s in order], at


def test_bit_equalities():
    pl, pr = canonical('left'), canonical('right')
    N, S = sum(Q.LENGTHS), len(Q.LENGTHS)
    keep = lambda r: type(r)(*[[None if t is None else t.clone() for t in f] if isinstance(f, list) else f for f in r])  # noqa: E731
    base = keep(run([pl, pr], Q.LENGTHS, 10))
    torch.cuda.synchronize()
    assert all(not torch.equal(bits(base.para[h][0]), bits(dev(p.init)[0])) for h, p in ((0, pl), (1, pr)))
    # (e) a repeat
    again = run([pl, pr], Q.LENGTHS, 10)
    assert all(same(hand(base, h), hand(again, h)) and torch.equal(base.seq_status[h], again.seq_status[h]) for h in (0, 1))
    # (c) hand slot 0 against hand slot 1; (d) hands = 1 is half of hands = 2
    swapped = run([pr, pl], Q.LENGTHS, 10)
    assert same(hand(swapped, 0), hand(base, 1)) and same(hand(swapped, 1), hand(base, 0))
    for h, prob in ((0, pl), (1, pr)):
        one = run(prob, Q.LENGTHS, 10)
        assert same(one, hand(base, h)) and torch.equal(one.seq_status, base.seq_status[h])
    # (b) every sequence alone (S = 1) against itself in slots 0 and 2 of a ragged batch of three
    st = Q.starts_of(Q.LENGTHS)
    for share in (True, False):
        ref = hand(base, 1) if share else run(pr, Q.LENGTHS, 10, share=False)
        for s in range(S):
            n = Q.LENGTHS[s]
            alone = run(rows_of(pr, slice(int(st[s]), int(st[s + 1]))), (n,), 10, share=share)
            assert same(alone, ref, rb=slice(int(st[s]), int(st[s + 1]))), (share, s)
            for order in ([s] + [x for x in range(S) if x != s], [x for x in range(S) if x != s] + [s]):
                prob, lengths, at = permuted(pr, order)
                moved = run(prob, lengths, 10, share=share)
                assert same(moved, alone, ra=slice(at[s], at[s] + n)), (share, s, order)
                assert moved.seq_status.tolist() == [0] * S
    # (f) 5 + 5 with the state against 10 (the prior stays centred on the first start)
    st10 = MF.new_seq_state(N, S, 2)
    whole = run([pl, pr], Q.LENGTHS, 10, state=st10)
    first = run([pl, pr], Q.LENGTHS, 5, state=True)
    second = run([pl, pr], Q.LENGTHS, 5, state=first.state, init=[t.clone() for t in first.para], anchor=[dev(pl.init), dev(pr.init)])
    fields = tuple(k for k in FIELDS if k != 'mse_before')
    live = [n for n in range(N) if n != Q.INERT]
    for h in (0, 1):
        assert same(hand(whole, h), hand(base, h)) and same(hand(whole, h), hand(second, h), fields, live, live)
        assert torch.equal(bits(st10.frames[h]), bits(second.state.frames[h])) and torch.equal(bits(st10.seq[h]), bits(second.state.seq[h]))
        assert st10.seq[h][:, 22].view(torch.int32).tolist() == [10] * S and st10.frames[h][:, 130].view(torch.int32).tolist() == [10] * 6 + [0] + [10] * 2
    # (h) p_out aliasing p0, (i) the inert frame's rows untouched: p0's bits, its state as it was
    p0 = [dev(pl.init), dev(pr.init)]
    seq_start = torch.tensor(Q.starts_of(Q.LENGTHS)).int().cuda()
    state = [torch.full((N, _capi.MANO_FIT_STATE), 7.0, device='cuda') for _ in (0, 1)]
    for t in state:
        t[live] = 0.0
    tabs, t_joints, t_conf = [tables(pl), tables(pr)], [dev(pl.joints), dev(pr.joints)], [dev(pl.joints_conf), dev(pr.joints_conf)]
    call = lambda init, out=None, state=None: F.mano_fit_sequence(tabs, init, seq_start, joints=t_joints, joints_conf=t_conf, iters=10, lr=pl.lr,  # noqa: E731
                                                                  weights=pl.weights, smooth=Q.SMOOTH, share_betas=True, para_out=out, state=state)
    al, _ = call(p0, p0, state)
    torch.cuda.synchronize()
    for h, prob in ((0, pl), (1, pr)):
        assert al[h]['para'] is p0[h] and torch.equal(bits(p0[h]), bits(base.para[h]))
        assert torch.equal(bits(p0[h][Q.INERT]), bits(dev(prob.init)[Q.INERT])) and bool((state[h][Q.INERT] == 7.0).all())
        assert torch.equal(bits(state[h][live]), bits(st10.frames[h][live]))
    # (g) a captured graph replay against the eager call
    init = [dev(pl.init), dev(pr.init)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(init)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, seq_status = call(init)
    graph.replay()
    torch.cuda.synchronize()
    for h in (0, 1):
        assert torch.equal(bits(out[h]['para']), bits(base.para[h])) and torch.equal(bits(out[h]['verts']), bits(base.verts[h]))
        assert torch.equal(bits(out[h]['mse']), bits(torch.cat([base.mse_before[h], base.mse_after[h]], 1))) and torch.equal(out[h]['status'], base.status[h])
        assert torch.equal(seq_status[h], base.seq_status[h])


SHAPES = {
    'T1': dict(lengths=(1,)), 'T2': dict(lengths=(2,)), 'T3': dict(lengths=(3,)),
    'no_data_at_both_ends': dict(lengths=(4, 2), no_data=(0, 3, 5)),
    'two_adjacent_inert_frames': dict(lengths=(6,), inert=(2, 3)),
    'a_sequence_of_inert_frames': dict(lengths=(2, 1, 2), inert=(2,)),
    'a_non_finite_target_in_use': dict(lengths=(3,), bad_target=1),
    'around_the_wave': dict(lengths=(WAVE - 1, WAVE, WAVE + 1), long=True),
    'one_below_the_lanes': dict(lengths=(LANES - 1,), long=True), 'the_lanes': dict(lengths=(LANES,), long=True),
    'one_above_the_lanes': dict(lengths=(LANES + 1,), long=True),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_shapes_where_the_kernels_can_go_wrong(name):
    """2 iterations, shared shape, one hand: no neighbour, one, both; no data at either end of a sequence; adjacent inert frames; a sequence with no usable
    frame (seq_status 2); a non-finite target in use (status 8); sequence lengths one below, at and one above the shape reduction's wave (64) and its
    width (DIR_MANO_FIT_SEQ_LANES = 256).  Against the float64 restatement at the canonical case's 2-iteration gates; S = 1 and S = 3.  The long cases
    hold the SHARED BETAS to that gate (they are what the reduction makes).  Their other outputs are the largest over hundreds of frames, not over 9, so
    the canonical record does not bound them: their gate is 4 x the float32-against-float64 difference of the restatement on the very same problem,
    measured here on the CPU -- never on the kernel."""
    spec = SHAPES[name]
    lengths = spec['lengths']
    prob, _ = Q.sequence_problem(lengths, 'right', 1, spec.get('no_data', ()), spec.get('inert', ()))
    if 'bad_target' in spec:
        jt = prob.joints.copy()
        jt[spec['bad_target'], 3, 1] = np.inf
        prob = prob._replace(joints=jt)
    ref = with_starts(Q.fit_sequence(prob, lengths, 2, torch.float64), lengths)
    got = run(prob, lengths, 2)
    torch.cuda.synchronize()
    worst, gates = {}, Q.GATES['shared'][2]
    if spec.get('long'):
        r32 = Q.fit_sequence(prob, lengths, 2, torch.float32)
        gates = dict({k: float((r32[k].double() - ref[k]).abs().max()) for k in R.OUTPUTS}, shape=gates['shape'])
    check_against(got, ref, gates, (name,), worst)
    for key, (d, g) in sorted(worst.items()):
        print(key, 'difference %.3g gate %.3g (%.2f of it)' % (d, g, d / g))
    for key, (d, g) in worst.items():
        assert d <= g, (key, d, g)
    if name == 'a_sequence_of_inert_frames':
        assert got.seq_status.tolist() == [0, MF.SEQ_STATUS_EMPTY, 0]
    if name == 'a_non_finite_target_in_use':
        assert got.status.tolist() == [0, MF.STATUS_NO_DATA, 0] and not torch.equal(bits(got.para[1]), bits(dev(prob.init)[1]))


def test_a_step_that_goes_non_finite_freezes_the_frame_where_its_neighbours_still_see_it():
    """w_joints 1e26: the first step's v overflows in every frame that has data (the float32 restatement freezes them at once for 1e24 .. 1e28 alike, and
    takes every step at 1e22), so those frames keep p0 with status bit 2 and an untouched state, while the two frames without data go on for all 6 iterations,
    pulled towards their frozen neighbours, and the shapes step on their prior alone.  Status words, step counts and the frozen rows against the restatement."""
    pl, pr = (canonical(s)._replace(weights=dict(canonical(s).weights, w_joints=1e26)) for s in ('left', 'right'))
    N, S = sum(Q.LENGTHS), len(Q.LENGTHS)
    for share in (True, False):
        state = MF.new_seq_state(N, S, 2)
        got = run([pl, pr], Q.LENGTHS, 6, share=share, state=state)
        torch.cuda.synchronize()
        for h, prob in enumerate((pl, pr)):
            ref = Q.fit_sequence(prob, Q.LENGTHS, 6, torch.float32, share=share)
            assert got.status[h].tolist() == ref['status'].tolist() == [4, 4, 0, 4, 4, 4, 2, 4, 0] and got.seq_status[h].tolist() == ref['seq_status'].tolist() == [0, 0, 0]
            assert state.frames[h][:, 130].view(torch.int32).tolist() == ref['state'][4].tolist() == [0, 0, 6, 0, 0, 0, 0, 0, 6]
            assert state.seq[h][:, 22].view(torch.int32).tolist() == ref['seq_state'][4].tolist() == ([6] * S if share else [0] * S)
            p0 = dev(prob.init)
            frozen = [0, 1, 3, 4, 5, 7]
            assert torch.equal(bits(got.para[h][frozen][:, :51]), bits(p0[frozen][:, :51])) and torch.equal(bits(got.para[h][frozen][:, 61:]), bits(p0[frozen][:, 61:]))
            assert share or torch.equal(bits(got.para[h][frozen]), bits(p0[frozen]))
            assert float(state.frames[h][frozen][:, :128].abs().max()) == 0.0
            live = [n for n in range(N) if n != Q.INERT]
            assert all(bool(torch.isfinite(getattr(got, k)[h][live]).all()) for k in ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after'))
            for n in Q.NO_DATA:
                assert not torch.equal(bits(got.para[h][n, 6:51]), bits(p0[n, 6:51]))


PATTERN = 0x7FC0BEEF                     # a NaN: what no case owns holds it


class Arena(object):
    """device buffers between guard floats, everything pre-filled with NaN"""
    def __init__(self, floats):
        self.buf = torch.full((floats,), PATTERN, dtype=torch.int32, device='cuda')
        self.used, self.guards = 0, []

    def take(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.guards.append((self.used, self.used + 16))
        t = self.buf[self.used + 16:self.used + 16 + n]
        self.used += 16 + n
        self.guards.append((self.used, self.used + 16))
        return t.view(dtype).view(*shape)

    def intact(self):
        return all(bool((self.buf[a:b] == PATTERN).all()) for a, b in self.guards) and bool((self.buf[self.used + 16:] == PATTERN).all())


def raw_call(prob, lengths, iters, out, work, work_bytes, smooth=Q.SMOOTH, seq_start=None, host=None, hands=1):
    N, S = prob.init.shape[0], len(lengths)
    w = prob.weights
    opts = _capi.ManoFitOpts(*[float(w.get(k, 0.0)) for k in F.MANO_FIT_WEIGHTS], (C.c_float * 4)(*prob.lr), 0.9, 0.999, 1e-8, iters)
    starts = [int(x) for x in Q.starts_of(lengths)]
    hostp = None if host is None else C.cast((C.c_int32 * (S + 1))(*host), C.POINTER(C.c_int32))
    sopts = _capi.ManoFitSeqOpts(smooth[0], smooth[1], smooth[2], 1, hostp, (C.c_void_p * 2)(None, None))
    keep = [dev(prob.init), dev(prob.joints), dev(prob.joints_conf), torch.tensor(starts if seq_start is None else seq_start, dtype=torch.int32).cuda()]
    P = _capi.ptr
    hd = _capi.ManoFitHand(P(keep[0]), None, P(out['para']), None, P(keep[1]), P(keep[2]), None, None, P(out['verts']), P(out['joints']), P(out['joint_uv']),
                           P(out['mse']), P(out['status']), None)
    rc = _capi.lib().dir_mano_fit_sequence((_capi.ManoTables * 1)(tables(prob)), (_capi.ManoFitHand * 1)(hd), C.byref(opts), C.byref(sopts), P(keep[3]), S, N, hands,
                                           P(out['seq_status']), C.c_void_p(work.data_ptr()), work_bytes, _capi.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_workspace_guards_and_refused_arguments():
    """the workspace is exactly what the query says (0xFF all over before the call, the bytes around it untouched after), the outputs sit between guard
    floats, and refused arguments return an error code and launch nothing"""
    prob, lengths = canonical('right'), Q.LENGTHS
    N, S = sum(lengths), len(lengths)
    need = F.mano_fit_sequence_workspace_bytes(N, S, 1)
    assert need > 0 and need % 4 == 0 and F.mano_fit_sequence_workspace_bytes(N, S, 2) > need and F.mano_fit_sequence_workspace_bytes(N + 1, S, 1) > need
    assert F.mano_fit_sequence_workspace_bytes(0, 1, 1) == 0 and F.mano_fit_sequence_workspace_bytes(3, 4, 1) == 0 and F.mano_fit_sequence_workspace_bytes(3, 1, 3) == 0

    def fresh():
        ar = Arena(N * (64 + 2334 + 63 + 42 + 6 + 1) + S + 16 * 16)
        out = {'para': ar.take(N, 64), 'verts': ar.take(N, 778, 3), 'joints': ar.take(N, 21, 3), 'joint_uv': ar.take(N, 21, 2), 'mse': ar.take(N, 6),
               'status': ar.take(N, dtype=torch.int32), 'seq_status': ar.take(S, dtype=torch.int32)}
        return ar, out, torch.full((need + 512,), 0xFF, dtype=torch.uint8, device='cuda')
    ar, out, buf = fresh()
    assert raw_call(prob, lengths, 10, out, buf[256:], need) == 0
    assert ar.intact() and bool((buf[:256] == 0xFF).all()) and bool((buf[256 + need:] == 0xFF).all())
    base = run(prob, lengths, 10)
    assert torch.equal(bits(out['para']), bits(base.para)) and torch.equal(bits(out['verts']), bits(base.verts)) and torch.equal(bits(out['joints']), bits(base.joints))
    assert torch.equal(bits(out['joint_uv']), bits(base.joint_uv)) and torch.equal(out['status'], base.status) and torch.equal(out['seq_status'], base.seq_status)
    assert torch.equal(bits(out['mse']), bits(torch.cat([base.mse_before, base.mse_after], 1)))
    good = [int(x) for x in Q.starts_of(lengths)]
    assert raw_call(prob, lengths, 10, out, buf[256:], need, host=good) == 0
    refused = (dict(work_bytes=need - 4), dict(host=[0, 4, 1, 9]), dict(host=[1, 1, 4, 9]), dict(host=[0, 1, 4, 8]), dict(smooth=(-1.0, 1.0, 1.0)),
               dict(smooth=(1.0, -1e-9, 1.0)), dict(smooth=(1.0, 1.0, float('nan'))), dict(hands=3))
    for kw in refused:
        ar, out, buf = fresh()
        rc = raw_call(prob, lengths, 10, out, buf[256:], kw.pop('work_bytes', need), **kw)
        assert rc == -1 and _capi.lib().dir_last_error().startswith(b'dir_mano_fit_sequence'), (kw, rc)
        assert ar.intact() and all(bool((bits(t) == PATTERN).all()) for t in out.values()) and bool((buf == 0xFF).all())       # nothing was launched
    # a seq_start on the device that breaks the rule cannot be checked without a host read: every index is clamped to the N frames
    ar, out, buf = fresh()
    assert raw_call(prob, lengths, 2, out, buf[256:], need, seq_start=[5, -3, 40, 2]) == 0
    assert ar.intact() and bool((buf[:256] == 0xFF).all()) and bool((buf[256 + need:] == 0xFF).all())


def test_python_surface():
    """fit_mano_sequence: layers or tables, one hand or a pair, start='closed' = start_mano then the fit anchored at its parameters; refused arguments"""
    from dir_amd.manopth.manolayer import ManoLayer
    pl, pr = canonical('left'), canonical('right')
    layers = [ManoLayer(root_rot_mode='6D', use_pca=True, robust_rot=True, ncomps=45, center_idx=R.CENTER, flat_hand_mean=False, side=s, seed=1234).cuda() for s in ('left', 'right')]
    kw = dict(iters=5, lr=0.03, weights=pr.weights)
    tg = dict(joints=[dev(pl.joints), dev(pr.joints)], joints_conf=[dev(pl.joints_conf), dev(pr.joints_conf)])
    init = [dev(pl.init), dev(pr.init)]
    want = run([pl, pr], Q.LENGTHS, 5)
    got = MF.fit_mano_sequence(layers, init, Q.LENGTHS, **tg, **kw)
    assert all(same(hand(got, h), hand(want, h)) for h in (0, 1)) and got.state is None
    # finite starts for the closed form (start_mano passes a non-finite row through; the sequence fit then finds it inert all the same)
    st = MF.start_mano(layers, init, **tg, weights=pr.weights)
    closed = MF.fit_mano_sequence(layers, init, Q.LENGTHS, start='closed', **tg, **kw)
    by_hand = MF.fit_mano_sequence(layers, st.para, Q.LENGTHS, anchor=st.para, **tg, **kw)
    assert all(same(hand(closed, h), hand(by_hand, h)) and not torch.equal(bits(closed.para[h][0]), bits(want.para[h][0])) for h in (0, 1))
    assert closed.status[1].tolist() == [0] * 6 + [2] + [0] * 2
    lean = MF.fit_mano_sequence(layers[1], init[1], Q.LENGTHS, joints=tg['joints'][1], joints_conf=tg['joints_conf'][1], outputs=False, **kw)
    assert lean.verts is None and torch.equal(bits(lean.para), bits(want.para[1])) and lean.seq_status.tolist() == [0, 0, 0]
    for bad in (dict(seq_lengths=(1, 3, 4)), dict(seq_lengths=(0, 4, 5)), dict(smooth={'wrist': 1.0}), dict(start='warm'), dict(smooth={'root': -1.0})):
        args = dict(dict(seq_lengths=Q.LENGTHS, joints=tg['joints'][1], joints_conf=tg['joints_conf'][1]), **bad)
        with pytest.raises((ValueError, _capi.DirHipError)):
            MF.fit_mano_sequence(layers[1], init[1], args.pop('seq_lengths'), **args, **kw)


@pytest.fixture(scope='module')
def state():
    from dir_amd import synth
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


def test_fit_mano_command_with_sequences(tmp_path, state):
    """apps.fit_mano --sequences on the canonical case, both sides (the checkpoint's MANO tables are the 'pca' tables of the cases): para_<side> = the
    library call's, betas_<side> and seq_status_<side>; --bs splits between sequences, never inside one; --per_frame_shape; without --sequences the keys
    are the old ones and seq_len is ignored"""
    from dir_amd.apps import fit_mano as A
    pl, pr = canonical('left'), canonical('right')
    tg = {'joints_left': pl.joints, 'joints_conf_left': pl.joints_conf, 'init_left': pl.init, 'joints_right': pr.joints, 'joints_conf_right': pr.joints_conf,
          'init_right': pr.init, 'seq_len': np.asarray(Q.LENGTHS)}
    np.savez(str(tmp_path / 'T.npz'), **tg)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    common = ['--model', ck, '--targets', str(tmp_path / 'T.npz'), '--iters', '5', '--lr', '0.03', '--center', str(R.CENTER), '--w_pca', '1e-3', '--w_beta', '1e-2']
    out = {}
    for name, extra in (('seq', ['--sequences']), ('split', ['--sequences', '--bs', '4']), ('frames', ['--sequences', '--per_frame_shape']), ('plain', [])):
        assert A.main(common + ['--out', str(tmp_path / (name + '.npz'))] + extra) == 18
        with np.load(str(tmp_path / (name + '.npz'))) as f:
            out[name] = {k: f[k] for k in f.files}
    new = sorted('%s_%s' % (k, s) for s in ('left', 'right') for k in ('betas', 'seq_status'))
    assert sorted(set(out['seq']) - set(out['plain'])) == new and set(out['plain']) <= set(out['seq'])
    assert sorted(out['plain']) == sorted('%s_%s' % (k, s) for s in ('left', 'right') for k in FIELDS)
    want = run([pl, pr], Q.LENGTHS, 5)
    for h, s in enumerate(('left', 'right')):
        assert np.array_equal(out['seq']['para_' + s], want.para[h].cpu().numpy(), equal_nan=True) and out['seq']['seq_status_' + s].tolist() == [0, 0, 0]
        assert out['seq']['status_' + s].tolist() == want.status[h].tolist() and out['seq']['betas_' + s].shape == (3, 10)
        assert np.array_equal(out['seq']['betas_' + s], out['seq']['para_' + s][[0, 1, 4], 51:61])
        assert all(np.array_equal(out['split'][k], out['seq'][k], equal_nan=True) for k in out['seq']), 'a batch boundary between sequences changes nothing'
        assert not np.array_equal(out['frames']['para_' + s][1, 51:61], out['frames']['para_' + s][3, 51:61])
        assert not np.array_equal(out['plain']['para_' + s][1], out['seq']['para_' + s][1])      # (frame 0 is a sequence of one: no neighbour, its own shape)
