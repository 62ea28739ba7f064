"""CPU-only: the restatement of dir_mano_fit_pair's rule (tests/helpers/mano_pair_fit_ref.py) is what it says it is, the constants the GPU test
(tests/test_gpu_mano_pair_fit.py) gates with are re-measured here -- on the restatement, never on the kernel -- and capsule_radii (dir_amd/utils/
mano_fit.py, plain torch) gives the radii of a constructed table.

Measured here (float64): the behaviour case 'separate' (anchor + collision only, 5 pairs, w_col 1e4, w_init 1e-2, w_off_init 1, lr 0.01 on root and PCA,
3e-3 on the offset): largest overlap 9.9, 18.3, 12.8, 17.2, 10.9 mm at the start -> 0 mm on every pair after 50 iterations (asserted: below half).
Branch margins of the three parity cases over 50 iterations: asserted >= H_MIN = 1e-6 m and S_MIN = 1e-5.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import mano_fit_ref as R  # noqa: E402
import mano_pair_fit_ref as P  # noqa: E402

F64 = torch.float64


def _pts(*rows):
    return [torch.tensor([r], dtype=F64) for r in rows]


def test_segment_distance_closed_forms():
    """parallel, crossing, end-to-end and point-like segments: s, t and d of the procedure against the values known in closed form"""
    # parallel, side by side, 0.3 apart: den = 0 -> s = 0, whose t falls below 0 -> t = 0 and s is clamped again; then s = 0 with t its projection
    g = P.segments(*_pts((0, 0, 0), (1, 0, 0), (0.25, 0.3, 0), (2, 0.3, 0)))
    assert float(g['s']) == 0.25 and float(g['t']) == 0.0 and abs(float(g['d']) - 0.3) < 1e-15
    g = P.segments(*_pts((0, 0, 0), (1, 0, 0), (-1, 0.3, 0), (3, 0.3, 0)))
    assert float(g['s']) == 0.0 and abs(float(g['t']) - 0.25) < 1e-15 and abs(float(g['d']) - 0.3) < 1e-15
    # crossing in the middle: d = 0 and no direction
    g = P.segments(*_pts((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)))
    assert abs(float(g['s']) - 0.5) < 1e-15 and abs(float(g['t']) - 0.5) < 1e-15 and float(g['d']) == 0.0 and not bool(torch.isfinite(g['n']).all())
    # skew lines whose common perpendicular meets both segments: d = the lines' distance
    g = P.segments(*_pts((-1, 0, 0), (1, 0, 0), (0.2, -1, 0.7), (0.2, 3, 0.7)))
    assert abs(float(g['s']) - 0.6) < 1e-15 and abs(float(g['t']) - 0.25) < 1e-15 and abs(float(g['d']) - 0.7) < 1e-15
    assert torch.allclose(g['n'], torch.tensor([[0.0, 0.0, -1.0]], dtype=F64))
    # end to end on one line with a gap of 0.5: the two facing end points
    g = P.segments(*_pts((0, 0, 0), (1, 0, 0), (1.5, 0, 0), (4, 0, 0)))
    assert float(g['s']) == 1.0 and float(g['t']) == 0.0 and abs(float(g['d']) - 0.5) < 1e-15
    # t clamped to 1, then s re-clamped
    g = P.segments(*_pts((0, 0, 0), (1, 0, 0), (3, 2, 0), (2, 1, 0)))
    assert float(g['s']) == 1.0 and float(g['t']) == 1.0 and abs(float(g['d']) - 2 ** 0.5) < 1e-15
    # point-like first segment, point-like second segment, both
    g = P.segments(*_pts((0.5, 1, 0), (0.5, 1, 1e-9), (0, 0, 0), (2, 0, 0)))
    assert float(g['s']) == 0.0 and abs(float(g['t']) - 0.25) < 1e-15 and abs(float(g['d']) - 1.0) < 1e-15
    g = P.segments(*_pts((0, 0, 0), (2, 0, 0), (0.5, 1, 0), (0.5, 1, 1e-9)))
    assert float(g['t']) == 0.0 and abs(float(g['s']) - 0.25) < 1e-15 and abs(float(g['d']) - 1.0) < 1e-15
    g = P.segments(*_pts((0, 0, 0), (0, 0, 1e-9), (0, 3, 4), (0, 3, 4)))
    assert float(g['s']) == 0.0 and float(g['t']) == 0.0 and abs(float(g['d']) - 5.0) < 1e-15
    # against a brute-force search over both parameters on random segments
    gen = torch.Generator().manual_seed(3)
    S = [torch.randn(40, 3, dtype=F64, generator=gen) for _ in range(4)]
    g = P.segments(*S)
    u = torch.linspace(0, 1, 401, dtype=F64)
    P1 = S[0][:, None, :] + u[None, :, None] * (S[1] - S[0])[:, None, :]
    P2 = S[2][:, None, :] + u[None, :, None] * (S[3] - S[2])[:, None, :]
    brute = torch.cdist(P1, P2).reshape(40, -1).min(1).values
    assert bool((g['d'] <= brute + 1e-12).all()) and float((brute - g['d']).max()) < 1e-3


def _col_energy(XL, XR, o, rad, k_col, s, t):
    """k_col / 2 * sum h^2 with s, t given (constants)"""
    pa, ch = list(P.PARENT), list(P.CHILD)
    XR = XR + o[:, None]
    A, B = XL[:, pa][:, :, None], XL[:, ch][:, :, None]
    C, D = XR[:, pa][:, None], XR[:, ch][:, None]
    w = (A + s[..., None] * (B - A)) - (C + t[..., None] * (D - C))
    d = torch.sqrt((w * w).sum(-1))
    h = torch.clamp((rad[0][:, None] + rad[1][None, :]) - d, min=0)
    return k_col / 2.0 * (h * h).sum()


def test_hand_written_gradient_is_autograd_with_s_and_t_detached():
    """the gather of step 2a (joint cotangents of both hands, g_o) against autograd of the one-scalar collision energy, s and t constants, to 1e-12"""
    pp = P.pair_problem('separate', 3)
    T = lambda x: torch.from_numpy(np.asarray(x)).double()  # noqa: E731
    ev = [R.residual_gradient(h, T(h.init), F64) for h in pp.hands]
    XL, XR, o = ev[0][1]['joints'].clone().requires_grad_(True), ev[1][1]['joints'].clone().requires_grad_(True), T(pp.o0).requires_grad_(True)
    rad, k_col = [T(r) for r in pp.radii], 2.0 * 1e4 / 400.0
    cl = P.collision(XL.detach(), XR.detach() + o.detach()[:, None], rad[0], rad[1], k_col)
    assert int(cl['active'].sum()) > 30 and not bool(cl['nodir'].any())
    E = _col_energy(XL, XR, o, rad, k_col, cl['s'], cl['t'])
    gL, gR, go = torch.autograd.grad(E, [XL, XR, o])
    scale = float(gL.abs().max())
    for got, want in ((cl['gL'], gL), (cl['gR'], gR), (cl['go'], go)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, scale)
    # the sum over the right end points is g_o, and the two hands' sums cancel
    assert float((cl['gR'].sum(1) - cl['go']).abs().max()) <= 1e-12 * scale and float((cl['gL'].sum(1) + cl['go']).abs().max()) <= 1e-12 * scale


def test_gradient_against_central_differences_of_E():
    """the rule's whole gradient (both hands' 64-vectors and o, priors included) against central finite differences of P.energy (s, t NOT held fixed:
    the envelope gradient is the true one away from the switches)"""
    pp = P.pair_problem('uv', 2)
    T = lambda x: torch.from_numpy(np.asarray(x)).double()  # noqa: E731
    p = [T(h.init).requires_grad_(True) for h in pp.hands]
    o = T(pp.o0).requires_grad_(True)
    E = P.energy(pp, p, o)
    g = torch.autograd.grad(E, p + [o])
    # the restatement's own gradient pieces: residuals + collision cotangents through the layer + priors
    k_col = 2.0 * pp.pair_weights['w_col'] / 400.0
    ev = [R.residual_gradient(h, p[i].detach(), F64) for i, h in enumerate(pp.hands)]
    cl = P.collision(ev[0][1]['joints'], ev[1][1]['joints'] + o.detach()[:, None], T(pp.radii[0]), T(pp.radii[1]), k_col)
    for i, h in enumerate(pp.hands):
        mine = ev[i][0] + P._extra_gradient(h, p[i].detach(), F64, cl['gL' if i == 0 else 'gR'])
        mine = mine + 2.0 * h.weights['w_init'] * (p[i].detach() - T(h.init))
        assert float((mine - g[i]).abs().max()) <= 1e-10 * max(1.0, float(g[i].abs().max()))
    assert float((cl['go'] - g[2]).abs().max()) <= 1e-10 * max(1.0, float(g[2].abs().max()))
    gen = np.random.RandomState(11)
    eps = 1e-6
    for _ in range(12):
        which, row = int(gen.randint(3)), int(gen.randint(2))
        comp = int(gen.randint(3 if which == 2 else 51))
        def at(delta):
            q = [x.detach().clone() for x in p] + [o.detach().clone()]
            q[which][row, comp] += delta
            return float(P.energy(pp, q[:2], q[2], detach_st=False))
        fd = (at(eps) - at(-eps)) / (2 * eps)
        an = float(g[which][row, comp])
        assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 1e-7, (which, row, comp, fd, an)


def test_without_coupling_terms_the_rule_is_mano_fit_ref():
    """w_col = 0, no offset terms, lr_o = 0: both hands are mano_fit_ref.fit's, bit for bit in float32, and the offset comes back as it went in"""
    pp = P.pair_problem('uv', 3)._replace(pair_weights={'w_col': 0.0, 'w_off': 0.0, 'w_off_init': 0.0}, lr_o=0.0)
    for dt in (torch.float32, F64):
        r = P.fit_pair(pp, 10, dt)
        for i, h in enumerate(pp.hands):
            ref = R.fit(h, 10, dt)
            assert all(torch.equal(r['hands'][i][k], ref[k]) for k in R.OUTPUTS + ('status', 'mse_before'))
            assert all(torch.equal(a, b) for a, b in zip(r['state'][i], ref['state']))
        assert torch.equal(r['offset'], torch.from_numpy(pp.o0).to(dt)) and r['pair_status'].tolist() == [0, 0, 0]
        assert bool((r['col'][:, 1] > 0).all())                  # the measure does not depend on w_col
    # hands 1 m apart: nothing is active, the same equality with w_col > 0
    far = P.pair_problem('uv', 3)._replace(o0=np.tile(np.float32([1.0, 0, 0]), (3, 1)), lr_o=0.0, pair_weights={'w_col': 1e3, 'w_off': 0.0, 'w_off_init': 0.0})
    r = P.fit_pair(far, 10, torch.float32)
    assert all(torch.equal(r['hands'][i]['para'], R.fit(h, 10, torch.float32)['para']) for i, h in enumerate(far.hands)) and float(r['col'].abs().max()) == 0.0


def test_energy_is_invariant_under_swapping_the_hand_slots():
    """E(p_L, p_R, o) = E with the slots exchanged and o -> -o, to 1e-12 (relative)"""
    for config in P.CONFIGS:
        pp = P.pair_problem(config, 3)
        T = lambda x: torch.from_numpy(np.asarray(x)).double()  # noqa: E731
        sw = pp._replace(hands=pp.hands[::-1], o0=-pp.o0, o_target=None if pp.o_target is None else -pp.o_target, radii=pp.radii[::-1])
        p = [T(h.init) for h in pp.hands]
        p = [x + 0.01 * torch.sin(torch.arange(x.numel(), dtype=F64).reshape(x.shape)) for x in p]
        o = T(pp.o0) + 0.003
        e1, e2 = float(P.energy(pp, p, o)), float(P.energy(sw, p[::-1], -o))
        assert abs(e1 - e2) <= 1e-12 * max(1.0, abs(e1)), (config, e1, e2)


def test_rows_pass_through_freeze_and_drop_the_coupling():
    pp = P.pair_problem('separate', 3)
    base = P.fit_pair(pp, 5, torch.float32)
    assert base['pair_status'].tolist() == [0, 0, 0] and not torch.equal(base['offset'], torch.from_numpy(pp.o0))
    # NaN in o0 of row 1: o passes through with its bits, the coupling is dropped (both hands as dir_mano_fit alone), the other rows unchanged
    o_bad = pp.o0.copy()
    o_bad[1, 2] = np.nan
    r = P.fit_pair(pp._replace(o0=o_bad), 5, torch.float32)
    assert r['pair_status'].tolist() == [0, 2, 0] and np.array_equal(r['offset'][1].numpy().view(np.uint32), o_bad[1].view(np.uint32))
    assert float(r['col'][1].abs().max()) == 0.0 and torch.equal(r['offset'][0], base['offset'][0])
    for i, h in enumerate(pp.hands):
        assert torch.equal(r['hands'][i]['para'][1], R.fit(h, 5, torch.float32)['para'][1]) and torch.equal(r['hands'][i]['para'][2], base['hands'][i]['para'][2])
    # NaN in the left hand's start of row 0: the hand passes through, the right hand is dir_mano_fit's, o stays
    bad = pp.hands[0].init.copy()
    bad[0, 9] = np.nan
    r = P.fit_pair(pp._replace(hands=(pp.hands[0]._replace(init=bad), pp.hands[1])), 5, torch.float32)
    assert r['pair_status'].tolist() == [1, 0, 0] and r['hands'][0]['status'].tolist() == [2, 0, 0]
    assert torch.equal(r['hands'][1]['para'][0], R.fit(pp.hands[1], 5, torch.float32)['para'][0]) and torch.equal(r['offset'][0], torch.from_numpy(pp.o0[0]))
    # a step of o that overflows (g * g is past float32 at once) is not taken: o stays at its last finite value, the hands go on
    hot = pp._replace(pair_weights=dict(pp.pair_weights, w_off_init=1e30), o_anchor=(pp.o0 + np.float32(1.0)).astype(np.float32))
    r = P.fit_pair(hot, 5, torch.float32)
    assert r['pair_status'].tolist() == [4, 4, 4] and bool(torch.isfinite(r['offset']).all()) and r['state'][2][4].tolist() == [0, 0, 0] and torch.equal(r['offset'], torch.from_numpy(pp.o0))
    assert [s.tolist() for s in (r['hands'][0]['status'], r['hands'][1]['status'])] == [[0, 0, 0], [0, 0, 0]] and r['state'][0][4].tolist() == [5, 5, 5]
    # crossing segments: energy in the report, no gradient, status bit 3
    X = torch.zeros(1, 21, 3, dtype=F64)
    X[0, :, 0] = torch.arange(21, dtype=F64) * 0.01
    Y = X.clone()
    Y[0, :, 0], Y[0, :, 1] = 0.005, (torch.arange(21, dtype=F64) - 10) * 0.01
    cl = P.collision(X, Y, torch.full((20,), 0.005, dtype=F64), torch.full((20,), 0.005, dtype=F64), 50.0)
    assert bool(cl['nodir'].any()) and float(cl['col'][0, 1]) == 0.01 and not bool((cl['active'] & cl['nodir']).any())


def test_state_resumes_bit_for_bit():
    pp = P.pair_problem('uv', 2)
    whole = P.fit_pair(pp, 10, torch.float32)
    first = P.fit_pair(pp, 5, torch.float32)
    # (the offset's anchor stays the first start: o_anchor defaults to o0, so it is given)
    second = P.fit_pair(pp._replace(o_anchor=pp.o0), 5, torch.float32, state=first['state'], init=[h['para'].numpy() for h in first['hands']],
                        anchor=[h.init for h in pp.hands], o0=first['offset'].numpy())
    a, b = P.flat(whole), P.flat(second)
    assert all(torch.equal(a[k][..., 2:] if k == 'col' else a[k], b[k][..., 2:] if k == 'col' else b[k]) for k in P.OUTPUTS)


def test_behaviour_the_overlap_halves():
    """anchor + collision only on five pairs whose capsules overlap at the start: the largest overlap falls below half its starting value on every pair"""
    pp = P.pair_problem('separate', 5)
    for dt in (F64, torch.float32):
        r = P.fit_pair(pp, 50, dt)
        print(dt, 'max overlap mm: start', [round(float(x) * 1e3, 2) for x in r['col'][:, 1]], 'end', [round(float(x) * 1e3, 2) for x in r['col'][:, 3]])
        assert bool((r['col'][:, 1] > 5e-3).all()) and bool((r['col'][:, 3] < 0.5 * r['col'][:, 1]).all())
        assert r['pair_status'].tolist() == [0] * 5


def test_branch_margins_of_the_parity_cases():
    """in the float64 run of every parity case no pair comes closer than H_MIN to h = 0 and no nearly active pair closer than S_MIN to a clamp switch,
    at any of the 51 evaluated iterates"""
    for config in P.CONFIGS:
        r = P.fit_pair(P.pair_problem(config, 3), 50, F64)
        print(config, 'h margin %.3g m, s margin %.3g' % (float(r['h_margin'].min()), float(r['s_margin'].min())))
        assert float(r['h_margin'].min()) >= P.H_MIN and float(r['s_margin'].min()) >= P.S_MIN, config
        assert r['pair_status'].tolist() == [0, 0, 0]


def test_float32_against_float64_runs_are_the_recorded_gates():
    """as tests/test_mano_fit_ref.py: a re-measured figure above its record fails, a record more than 4 x the re-measured figure is stale"""
    for config in P.CONFIGS:
        got = P.measure(config)
        for it in P.ITERS:
            print(config, it, {k: '%.3g (record %.3g)' % (got[it][k], P.GATES[config][it][k]) for k in P.OUTPUTS})
            for k in P.OUTPUTS:
                rec = P.GATES[config][it][k]
                assert got[it][k] <= rec, (config, it, k, got[it][k], rec)
                assert got[it][k] >= rec / 4.0, ('stale record', config, it, k, got[it][k], rec)


class _Table(dict):
    pass


def test_capsule_radii_on_cylinders():
    """a constructed table: the 21 template joints on five straight fingers, every vertex on a cylinder of known radius about the bone of the chain joint
    that owns it (one-hot skinning weights): capsule_radii returns those radii for any q; a bone whose parent joint owns no vertex gets 0"""
    from dir_amd.utils import mano_fit as MF
    reorder, tips = MF._REORDER, MF._TIPS['right']
    out_j = np.zeros((21, 3))
    for f in range(5):
        for k in range(4):
            out_j[1 + 4 * f + k] = (0.02 * (f - 2), 0.03 * (k + 1), 0.0)
    chain_j = np.zeros((16, 3))
    for o, src in enumerate(reorder):
        if src < 16:
            chain_j[src] = out_j[o]
    want = np.array([0.004 + 0.0005 * k for k in range(20)])
    want[[0, 4, 8, 12, 16]] = 0.0                                  # the wrist owns no vertex below
    v = np.zeros((778, 3))
    w = np.zeros((778, 16))
    free = [i for i in range(778) if i not in tips]
    bones = [k for k in range(20) if want[k] > 0]
    for n, i in enumerate(free):
        k = bones[n % len(bones)]
        a, b = out_j[MF.BONE_PARENT[k]], out_j[k + 1]
        ang, u = 0.7 * n, ((n // len(bones)) % 10) / 9.0
        v[i] = a + u * (b - a) + want[k] * np.array([np.cos(ang), 0.0, np.sin(ang)])          # the fingers run along y
        w[i, reorder[MF.BONE_PARENT[k]]] = 1.0
    for f, i in enumerate(tips):
        v[i] = out_j[4 + 4 * f]
        w[i, reorder[3 + 4 * f]] = 0.6                             # a fingertip vertex belongs to the last chain joint, at distance 0 from its bone
        w[i, 0] = 0.4
    # a regressor that returns the chain joints from the template: one helper vertex per joint would disturb the cylinders, so solve for it
    jr = chain_j @ np.linalg.pinv(v)
    assert np.abs(jr @ v - chain_j).max() < 1e-12
    tab = _Table(th_v_template=torch.from_numpy(v), th_weights=torch.from_numpy(w), th_J_regressor=torch.from_numpy(jr), side='right')
    # the five fingertip vertices sit ON their bones (distance 0): the largest distance (q = 1) is the cylinder's radius on every bone
    got = MF.capsule_radii(tab, q=1.0).double().numpy()
    assert got.shape == (20,) and np.abs(got - want).max() < 1e-7, (got, want)
    mid = MF.capsule_radii(tab, q=0.5).double().numpy()
    assert np.abs(mid - want).max() < 1e-7
