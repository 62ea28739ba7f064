"""GPU: dir_mano_fit_pair (csrc/mano_fit_pair.hip) -- both hands of a pair fitted together with the offset between them and a capsule collision
term -- against the float64 restatement of its rule (tests/helpers/mano_pair_fit_ref.py), its bit equalities with dir_mano_fit, and the behaviour
case (the overlap falls below half).

Gates: |kernel - float64 restatement| <= 4 x the largest |float32 restatement - float64 restatement| that tests/test_mano_pair_fit_ref.py measured on
the CPU for that configuration, iteration count and output (mano_pair_fit_ref.GATES); nothing here is measured on the kernel.  Every figure is
printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import mano_fit_ref as R  # noqa: E402
import mano_gpu_run as G  # noqa: E402
import mano_pair_fit_ref as P  # noqa: E402

from dir_amd import functional as F  # noqa: E402
from dir_amd.utils import mano_fit as MF  # noqa: E402

pytestmark = pytest.mark.gpu
HAND_FIELDS = ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after', 'status')
_REF = {}


def ref64(config, iters):
    """the float64 restatement on pair_problem(config, 3): computed once, shared, not to be written to"""
    if (config, iters) not in _REF:
        _REF[(config, iters)] = P.fit_pair(P.pair_problem(config, 3), iters, torch.float64)
    return _REF[(config, iters)]


def tables(prob):
    return G.packed(R.KIND, prob.side, prob.center, prob.root_palm)


def dev(a, rows=None):
    if a is None:
        return None
    a = np.asarray(a, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).cuda()


def run(pp, iters, rows=None, state=None, init=None, anchor=None, o0=None, o_anchor=None, pair_weights=None, lr_o=None):
    """fit_mano_pair on a PairProblem -> PairFitResult of device tensors"""
    hs = pp.hands
    arg = lambda k: [dev(getattr(h, k), rows) for h in hs]  # noqa: E731
    w = dict(hs[0].weights, **(pp.pair_weights if pair_weights is None else pair_weights))
    lr = dict(zip(MF.GROUPS, hs[0].lr), offset=pp.lr_o if lr_o is None else lr_o)
    return MF.fit_mano_pair([tables(h) for h in hs], arg('init') if init is None else init, dev(pp.o0, rows) if o0 is None else o0,
                            radii=[dev(r) for r in pp.radii], offset_target=dev(pp.o_target, rows), offset_conf=dev(pp.o_conf, rows),
                            offset_anchor=dev(pp.o_anchor, rows) if o_anchor is None else o_anchor, verts=arg('verts'), joints=arg('joints'),
                            joints_conf=arg('joints_conf'), joint_uv=arg('joint_uv'), uv_conf=arg('uv_conf'), iters=iters, lr=lr, weights=w, state=state, anchor=anchor)


def single(prob, iters, rows=None, state=None, init=None, anchor=None):
    """dir_mano_fit on one hand of a pair problem"""
    arg = lambda k: dev(getattr(prob, k), rows)  # noqa: E731
    return MF.fit_mano(tables(prob), arg('init') if init is None else init, arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'),
                       iters=iters, lr=dict(zip(MF.GROUPS, prob.lr)), weights=prob.weights, state=state, anchor=anchor)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def hand(res, h):
    return MF.FitResult(*[None if f is None else f[h] for f in res[:8]])


def same_hand(a, b, fields=HAND_FIELDS, row_a=None, row_b=None):
    pick = lambda t, r: bits(t) if r is None else bits(t)[r]  # noqa: E731
    return all(torch.equal(pick(getattr(a, k), row_a), pick(getattr(b, k), row_b)) for k in fields)


def same_pair(a, b, hand_fields=HAND_FIELDS):
    return (all(same_hand(hand(a, h), hand(b, h), hand_fields) for h in (0, 1)) and torch.equal(bits(a.offset), bits(b.offset))
            and torch.equal(a.pair_status, b.pair_status))


@pytest.mark.parametrize('config', P.CONFIGS)
def test_trajectory_parity_with_the_float64_restatement(config):
    """iters 1, 2, 10, 50 on 3 pairs: p of both hands, o, V, J, U at the returned iterate and the collision report inside 4 x the CPU-recorded
    float32-against-float64 differences; every status equal exactly"""
    pp = P.pair_problem(config, 3)
    worst = {}
    for it in P.ITERS:
        got = run(pp, it)
        torch.cuda.synchronize()
        ref = ref64(config, it)
        assert got.pair_status.tolist() == ref['pair_status'].tolist()
        for h in (0, 1):
            assert got.status[h].tolist() == ref['hands'][h]['status'].tolist()
        flat = {k: torch.stack([getattr(got, k)[0], getattr(got, k)[1]]) for k in ('para', 'verts', 'joints', 'joint_uv')}
        flat.update(offset=got.offset, col=got.collision)
        want = P.flat(ref)
        for k in P.OUTPUTS:
            worst[(it, k)] = (float((flat[k].double().cpu() - want[k]).abs().max()), P.gate(config, it, k))
    for key, (d, g) in sorted(worst.items()):
        print(config, key, 'difference %.3g gate %.3g (%.2f of it)' % (d, g, d / g))
    for key, (d, g) in worst.items():
        assert d <= g, (config, key, d, g)


def test_without_coupling_both_hands_are_dir_mano_fit_bit_for_bit():
    """w_col = 0, no offset terms, lr_o = 0: every output and state of both hands equals dir_mano_fit's and offset_out = o0; the same with w_col > 0 and
    the hands 1 m apart (inactive pairs are skipped, never added as zeros)"""
    for config in ('uv', 'joints'):
        pp = P.pair_problem(config, 3)._replace(o_target=None, o_conf=None)
        off = {'w_col': 0.0, 'w_off': 0.0, 'w_off_init': 0.0}
        far = dev(np.tile(np.float32([1.0, 0.0, 0.0]), (3, 1)))
        for o0, pw in ((None, off), (far, dict(off, w_col=1e4))):
            got = run(pp, 10, state=True, pair_weights=pw, lr_o=0.0, o0=o0)
            torch.cuda.synchronize()
            for h, prob in enumerate(pp.hands):
                alone = single(prob, 10, state=True)
                assert same_hand(hand(got, h), alone), (config, h)
                assert torch.equal(bits(got.state[h]), bits(alone.state))
                assert not torch.equal(bits(alone.para), bits(dev(prob.init)))
            assert torch.equal(bits(got.offset), bits(dev(pp.o0) if o0 is None else o0)) and got.pair_status.tolist() == [0, 0, 0]
            if o0 is None:
                assert bool((got.collision[:, 1] > 0).all())         # the measure does not depend on w_col
            else:
                assert float(got.collision.abs().max()) == 0.0


def test_bit_equalities_of_the_pair_fit():
    pp = P.pair_problem('separate', 5)
    keep = lambda r: MF.PairFitResult(*[[None if t is None else t.clone() for t in f] if isinstance(f, list) else (None if f is None else f.clone()) for f in r[:11]], None)  # noqa: E731
    base = keep(run(pp, 10))
    torch.cuda.synchronize()
    assert not torch.equal(bits(base.offset), bits(dev(pp.o0))) and bool((base.collision[:, 3] < base.collision[:, 1]).all())
    # a repeat run
    assert same_pair(base, run(pp, 10))
    # a pair alone against slot 3 of the batch of 5
    alone = run(pp, 10, rows=[3])
    for h in (0, 1):
        assert same_hand(hand(alone, h), hand(base, h), row_a=0, row_b=3)
    assert torch.equal(bits(alone.offset)[0], bits(base.offset)[3]) and torch.equal(bits(alone.collision)[0], bits(base.collision)[3])
    # 5 + 5 iterations with the state against 10
    st10 = ([MF.new_state(5), MF.new_state(5)], MF.new_offset_state(5))
    whole = run(pp, 10, state=st10)
    first = run(pp, 5, state=True)
    second = run(pp, 5, state=(first.state, first.offset_state), init=[t.clone() for t in first.para], anchor=[dev(h.init) for h in pp.hands],
                 o0=first.offset.clone(), o_anchor=dev(pp.o0))
    fields = tuple(k for k in HAND_FIELDS if k != 'mse_before')
    assert same_pair(whole, second, fields) and same_pair(whole, base)
    assert torch.equal(bits(whole.collision[:, 2:]), bits(second.collision[:, 2:])) and torch.equal(bits(whole.collision), bits(base.collision))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(st10[0] + [st10[1]], list(second.state) + [second.offset_state]))
    assert st10[1][:, 8].view(torch.int32).tolist() == [10] * 5 and st10[0][1][:, 130].view(torch.int32).tolist() == [10] * 5
    # a graph's replay against the eager call
    args = dict(radii=[dev(r) for r in pp.radii], iters=10, lr=dict(zip(MF.GROUPS, pp.hands[0].lr), offset=pp.lr_o), weights=dict(pp.hands[0].weights, **pp.pair_weights))
    tabs, p0, o0 = [tables(h) for h in pp.hands], [dev(h.init) for h in pp.hands], dev(pp.o0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        MF.fit_mano_pair(tabs, p0, o0, **args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = MF.fit_mano_pair(tabs, p0, o0, **args)
    graph.replay()
    torch.cuda.synchronize()
    assert same_pair(captured, base) and torch.equal(bits(captured.collision), bits(base.collision))
    # p_out aliasing p0 and offset_out aliasing o0
    w, pw = pp.hands[0].weights, pp.pair_weights
    res, pr = F.mano_fit_pair(tabs, p0, o0, [dev(r) for r in pp.radii], iters=10, lr=pp.hands[0].lr, lr_offset=pp.lr_o, weights=w, pair_weights=pw,
                              anchor=[dev(h.init) for h in pp.hands], offset_anchor=dev(pp.o0), para_out=p0, offset_out=o0)
    torch.cuda.synchronize()
    assert res[0]['para'] is p0[0] and pr['offset'] is o0
    assert all(torch.equal(bits(p0[h]), bits(base.para[h])) for h in (0, 1)) and torch.equal(bits(o0), bits(base.offset))
    # lr_o = 0 keeps o bit for bit while the hands move
    fixed = run(pp, 10, lr_o=0.0)
    assert torch.equal(bits(fixed.offset), bits(dev(pp.o0))) and not torch.equal(bits(fixed.para[0]), bits(dev(pp.hands[0].init)))


def test_inert_hand_nan_offset_and_frozen_offset():
    pp = P.pair_problem('uv', 3)
    base = run(pp, 10)
    # an inert left hand in row 1: its partner is dir_mano_fit's on that hand alone, o passes through, the other rows are untouched
    bad = pp.hands[0].init.copy()
    bad[1, 20] = np.nan
    got = run(pp._replace(hands=(pp.hands[0]._replace(init=bad), pp.hands[1])), 10)
    alone = single(pp.hands[1], 10)
    torch.cuda.synchronize()
    assert got.pair_status.tolist() == [0, 1, 0] and got.status[0].tolist()[1] == 2
    assert same_hand(hand(got, 1), alone, row_a=1, row_b=1) and np.array_equal(got.para[0][1].cpu().numpy().view(np.uint32), bad[1].view(np.uint32))
    assert torch.equal(bits(got.offset)[1], bits(dev(pp.o0))[1]) and float(got.collision[1].abs().max()) == 0.0
    for r in (0, 2):
        assert all(same_hand(hand(got, h), hand(base, h), row_a=r, row_b=r) for h in (0, 1)) and torch.equal(bits(got.offset)[r], bits(base.offset)[r])
    # a NaN in o0 of row 2 leaves o and drops the coupling: both hands as dir_mano_fit fits them alone
    o_bad = pp.o0.copy()
    o_bad[2, 0] = np.nan
    got = run(pp._replace(o0=o_bad), 10)
    torch.cuda.synchronize()
    assert got.pair_status.tolist() == [0, 0, 2] and np.array_equal(got.offset[2].cpu().numpy().view(np.uint32), o_bad[2].view(np.uint32))
    for h, prob in enumerate(pp.hands):
        assert same_hand(hand(got, h), single(prob, 10), row_a=2, row_b=2) and same_hand(hand(got, h), hand(base, h), row_a=0, row_b=0)
    # a non-finite radius does the same to every pair
    rad = (pp.radii[0].copy(), pp.radii[1])
    rad[0][7] = np.inf
    got = run(pp._replace(radii=rad), 10)
    assert got.pair_status.tolist() == [2, 2, 2] and all(same_hand(hand(got, h), single(prob, 10)) for h, prob in enumerate(pp.hands))
    # a step of o that overflows is not taken: o stays, status bit 2, the hands go on; the statuses are the restatement's
    hot = pp._replace(pair_weights=dict(pp.pair_weights, w_off_init=1e30), o_anchor=(pp.o0 + np.float32(1.0)).astype(np.float32))
    got, ref = run(hot, 5), P.fit_pair(hot, 5, torch.float32)
    torch.cuda.synchronize()
    assert got.pair_status.tolist() == ref['pair_status'].tolist() == [4, 4, 4] and torch.equal(bits(got.offset), bits(dev(pp.o0)))
    assert [got.status[h].tolist() for h in (0, 1)] == [ref['hands'][h]['status'].tolist() for h in (0, 1)] == [[0, 0, 0], [0, 0, 0]]
    assert not torch.equal(bits(got.para[0]), bits(dev(pp.hands[0].init)))


def test_zero_iterations_are_the_measure_alone():
    """iters = 0: parameters and offset come back bit for bit, col's two halves are equal and equal the restatement's report inside its gate"""
    pp = P.pair_problem('separate', 5)
    got = run(pp, 0)
    ref = P.fit_pair(pp, 0, torch.float64)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(got.para[h]), bits(dev(pp.hands[h].init))) for h in (0, 1)) and torch.equal(bits(got.offset), bits(dev(pp.o0)))
    assert torch.equal(bits(got.collision[:, :2]), bits(got.collision[:, 2:])) and got.pair_status.tolist() == [0] * 5
    d = float((got.collision.double().cpu() - ref['col']).abs().max())
    print('col at iters 0: difference %.3g, gate %.3g' % (d, P.gate('separate', 1, 'col')))
    assert d <= P.gate('separate', 1, 'col')


def test_behaviour_the_overlap_halves_on_the_device():
    """the CPU behaviour case (anchor + collision only, five overlapping pairs, 50 iterations): max h below half its starting value on every pair"""
    pp = P.pair_problem('separate', 5)
    got = run(pp, 50)
    torch.cuda.synchronize()
    col = got.collision.cpu()
    print('max overlap mm: start', [round(float(x) * 1e3, 2) for x in col[:, 1]], 'end', [round(float(x) * 1e3, 2) for x in col[:, 3]])
    assert bool((col[:, 1] > 5e-3).all()) and bool((col[:, 3] < 0.5 * col[:, 1]).all())
    assert got.pair_status.tolist() == [0] * 5 and all(got.status[h].tolist() == [0] * 5 for h in (0, 1))
