"""GPU: the guarded AdamW step (dir_grad_guard / dir_adamw_guarded_step, FlatAdamW(max_grad_norm, skip_nonfinite, ema_decay)) against the
numpy restatement tests/helpers/guarded_step_ref.py (itself pinned against torch by tests/test_guarded_step_ref.py) and torch on the CPU.

Tolerances, none taken from the code under test:
  norm         |norm - float64 numpy| / norm <= 1e-12: the products of float32 values are exact in double, the sums are log-depth in double
               (error ~ 1e-14 at these sizes); 6e-8 would be needed to move the float coefficient
  coefficient  1 float ulp against the restatement
  p, m, v, e   2e-7 (conftest.relerr), the project's fp32 bound, given the kernel's published coefficient
  everything the rule says stays: bit for bit
Buffers handed to the C ABI sit between canary floats that must survive."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import relerr
from dir_amd import _capi
from dir_amd import optim as DO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import guarded_step_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(64, 3, 7, 7), (64,), (5, 3), (1,), (21, 128, 128), (1027,)]
F32 = np.float32
CANARY, PAD = 1234.5, 64                       # 64 floats = 256 bytes on either side: the views keep 16-byte alignment
TRIP = 4 * 256 * 4096                          # elements of one grid-stride trip of the full grid
SIZES = [1, 3, 4, 5, 1027, TRIP + 7]


class Canaried(object):
    """n elements of `dtype` between two runs of canaries"""

    def __init__(self, n, dtype=torch.float32, data=None):
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device='cuda')
        self.t = self.buf[PAD:PAD + n]
        if data is None:
            self.t.zero_()
        else:
            self.t.copy_(torch.as_tensor(data))

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.t.numel():] == CANARY).all())


class Guard(object):
    """the device state and workspace of dir_grad_guard for gradients of n elements, both canaried"""

    def __init__(self, n, applied=0):
        L = _capi.lib()
        self.n = n
        self.ws = Canaried(L.dir_grad_norm_workspace_bytes(n) // 8, torch.float64)
        self.state = Canaried(ctypes.sizeof(_capi.GuardState) // 8, torch.float64)
        st = _capi.GuardState(applied=applied, coef=1.0)
        self.state.t.view(torch.uint8).copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))

    def run(self, g, max_norm=math.inf, skip=False):
        _capi.check(_capi.lib().dir_grad_guard(_capi.ptr(g), self.n, max_norm, int(skip), 0.9, 0.999, _capi.ptr(self.ws.t), self.ws.t.numel() * 8,
                                               _capi.ptr(self.state.t), None), 'dir_grad_guard')
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        assert self.ws.intact() and self.state.intact()
        return _capi.GuardState.from_buffer_copy(self.state.t.view(torch.uint8).cpu().numpy().tobytes())


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def mixed_grad(rng, n):
    return (rng.normal(0, 1, n) * 10.0 ** rng.randint(-4, 1, n)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize('n', SIZES)
def test_norm_equals_float64_numpy_and_repeats_its_bits(n):
    g_np = mixed_grad(np.random.RandomState(n % 1000), n)
    g = Canaried(n, data=g_np)
    guard = Guard(n)
    a = guard.run(g.t)
    b = guard.run(g.t)
    want = math.sqrt(float(np.sum(g_np.astype(np.float64) ** 2)))
    err = abs(a.norm - want) / want
    print('n %d: norm %.17g, float64 numpy %.17g, relative difference %.3g' % (n, a.norm, want, err))
    assert err <= 1e-12
    assert a.nonfinite == 0 and a.skip == 0 and a.coef == 1.0 and (a.applied, b.applied, b.skipped) == (1, 2, 0)
    assert np.float64(a.sumsq).tobytes() == np.float64(b.sumsq).tobytes() and np.float64(a.norm).tobytes() == np.float64(b.norm).tobytes()
    assert g.intact() and np.array_equal(g.t.cpu().numpy(), g_np)


def test_norm_sees_a_value_that_only_the_tail_holds():
    for n in (1027, TRIP + 7):                                            # n % 4 == 3: the last three elements are the tail
        g = Canaried(n)
        g.t[n - 1] = 3.0e4
        st = Guard(n).run(g.t, max_norm=1.0)
        assert st.norm == 3.0e4 and st.coef == G.clip_coef(9.0e8, 1.0) and g.intact()


def test_a_gradient_of_1e30_has_a_finite_norm():
    n = 1027
    g_np = np.zeros(n, F32)
    g_np[[0, 500, 1026]] = 1e30                                          # its float square is inf
    st = Guard(n).run(Canaried(n, data=g_np).t, max_norm=1.0, skip=True)
    want = math.sqrt(float(np.sum(g_np.astype(np.float64) ** 2)))
    assert math.isfinite(st.norm) and abs(st.norm - want) / want <= 1e-12 and st.nonfinite == 0 and st.skip == 0
    assert st.coef > 0 and ulps(st.coef, G.clip_coef(want * want, 1.0)) <= 1 and st.applied == 1 and st.clipped == 1


def test_one_nan_or_inf_anywhere_sets_nonfinite():
    n = 1027
    g_np = mixed_grad(np.random.RandomState(3), n)
    guard = Guard(n)
    g = Canaried(n, data=g_np)
    assert guard.run(g.t, skip=True).nonfinite == 0
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for pos in (0, n // 2, n - 1):                                    # n - 1 is in the tail
            g.t.copy_(torch.from_numpy(g_np))
            g.t[pos] = bad
            st = guard.run(g.t, skip=True)
            k += 1
            assert st.nonfinite == 1 and st.skip == 1 and (st.applied, st.skipped, st.skipped_in_row) == (1, k, k), (bad, pos)
    g.t.copy_(torch.from_numpy(g_np))
    st = guard.run(g.t, skip=True)
    assert st.nonfinite == 0 and (st.applied, st.skipped, st.skipped_in_row) == (2, k, 0)


@pytest.mark.parametrize('n', SIZES)
def test_one_guarded_step_between_canaries(n):
    """every size class of the update kernel (tail only, vectors + tail, more than one grid-stride trip), with the average"""
    rng = np.random.RandomState(n % 997)
    p0, g0 = rng.normal(0, 0.1, n).astype(F32), mixed_grad(rng, n)
    m0, v0 = rng.normal(0, 0.01, n).astype(F32), (rng.normal(0, 0.01, n) ** 2).astype(F32)
    e0 = rng.normal(0, 0.1, n).astype(F32)
    bufs = [Canaried(n, data=x) for x in (p0, g0, m0, v0, e0)]
    guard = Guard(n, applied=4)
    st = guard.run(bufs[1].t, max_norm=0.5)
    args = [_capi.ptr(b.t) for b in bufs] + [n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.75, _capi.ptr(guard.state.t), None]
    _capi.check(_capi.lib().dir_adamw_guarded_step(*args), 'dir_adamw_guarded_step')
    torch.cuda.synchronize()
    ref = G.new_state()
    ref['applied'] = 4
    p, m, v, e = G.guarded_step([p0], [g0], [m0], [v0], [e0], ref, 1e-3, max_norm=0.5, ema_decay=0.75, coef=st.coef)
    assert ulps(st.coef, ref['clip_coef']) <= 1 and st.applied == 5
    for b, want, name in zip(bufs, (p[0], g0, m[0], v[0], e[0]), 'pgmve'):
        assert b.intact(), name
        assert relerr(b.t.cpu().numpy(), want) < 2e-7, name
    assert np.array_equal(bufs[1].t.cpu().numpy(), g0) and guard.state.intact()


# ------------------------------------------------------------------------------------------------------------------------------ FlatAdamW
def make_params(rng):
    return [rng.normal(0, 0.1, s).astype(F32) for s in SHAPES]


def make_opt(p_np, lr=1e-3, **kw):
    ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in p_np]
    return ps, DO.FlatAdamW([{'params': ps, 'initial_lr': lr}], lr, **kw)


def draw_grads(rng):
    return [(rng.normal(0, 1, s) * 10.0 ** rng.randint(-4, 1)).astype(F32) for s in SHAPES]


def give(ps, gs):
    for p, g in zip(ps, gs):
        p.grad.copy_(torch.from_numpy(g))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def snapshot(opt):
    return [bits(t) for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq) + ((opt.flat_ema,) if opt.flat_ema is not None else ())]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('kw', [dict(skip_nonfinite=True), dict(max_grad_norm=1e30)], ids=['max_norm_inf', 'max_norm_far_above'])
def test_without_clipping_the_guarded_path_is_dir_adamw_step_bit_for_bit(kw):
    rng = np.random.RandomState(11)
    p_np = make_params(rng)
    ps_a, plain = make_opt(p_np)
    ps_b, guarded = make_opt(p_np, **kw)
    assert not plain.guarded and guarded.guarded and guarded.flat_ema is None
    for step in range(7):
        gs = draw_grads(rng)
        give(ps_a, gs); give(ps_b, gs)
        plain.step(); guarded.step()
        assert same(snapshot(plain), snapshot(guarded)), step
    st = guarded.guard_stats()
    assert (st['applied'], st['skipped'], st['clipped'], st['clip_coef']) == (7, 0, 0, 1.0) and guarded.step_count == plain.step_count == 7


def test_clipping_against_the_restatement_and_torch():
    rng = np.random.RandomState(12)
    decay, lr = 0.9, 1e-3
    p_np = make_params(rng)
    ps, opt = make_opt(p_np, lr, max_grad_norm=1.0, ema_decay=decay)
    tp = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p_np]
    ref = torch.optim.AdamW(tp, lr)
    tema = [t.detach().clone() for t in tp]
    p, m, v = [x.copy() for x in p_np], [np.zeros(s, F32) for s in SHAPES], [np.zeros(s, F32) for s in SHAPES]
    e = [x.copy() for x in p_np]
    rs = G.new_state()
    exact = [np.zeros(s, F32) for s in SHAPES]
    exact[0].reshape(-1)[5] = 2.0                                          # norm == max_norm == 2 exactly
    plan = [(draw_grads(rng), 1.0) for _ in range(7)] + [(exact, 2.0)] + [None] + [(draw_grads(rng), 1.0) for _ in range(2)]
    seen = set()
    for k, item in enumerate(plan):
        if item is None:                                                   # continue from a step count of 1000, loaded through load_state_dict
            sd = opt.state_dict()
            for s in sd['state'].values():
                s['step'] = torch.tensor(1000.0)
            opt.load_state_dict(sd)
            tsd = ref.state_dict()
            for s in tsd['state'].values():
                s['step'] = torch.tensor(1000.0)
            ref.load_state_dict(tsd)
            rs['applied'] = 1000
            assert opt.guard_stats()['applied'] == 1000
            continue
        gs, max_norm = item
        opt.configure(max_norm, False, decay)
        give(ps, gs)
        opt.step()
        st = opt.guard_stats()
        coef = F32(st['clip_coef'])
        p, m, v, e = G.guarded_step(p, gs, m, v, e, rs, lr, max_norm=max_norm, ema_decay=decay, coef=coef)
        d = ulps(coef, rs['clip_coef'])
        print('step %d: norm %.9g, coefficient %.9g (restatement %.9g, %d ulp)' % (k, st['grad_norm'], coef, rs['clip_coef'], d))
        assert d <= 1 and abs(st['grad_norm'] - rs['grad_norm']) <= 1e-12 * rs['grad_norm']
        assert st['applied'] == rs['applied'] and st['clipped'] == rs['clipped']
        seen.add(bool(coef < 1))
        for t, g in zip(tp, gs):
            t.grad = torch.from_numpy(g.copy()).mul_(float(coef))          # torch with the kernel's coefficient
        ref.step()
        with torch.no_grad():
            for a, b in zip(tema, tp):
                a.lerp_(b.detach(), 1 - decay)
        for i, (q, o) in enumerate(zip(ps, opt.offsets)):
            sl = slice(o, o + q.numel())
            got = [t[sl].cpu().numpy().reshape(SHAPES[i]) for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.flat_ema)]
            for have, want, name in zip(got, (p[i], m[i], v[i], e[i]), 'pmve'):
                assert relerr(have, want) < 2e-7, (k, i, name)
            assert relerr(got[0], tp[i].detach().numpy()) < 2e-7 and relerr(got[3], tema[i].numpy()) < 2e-7, (k, i)
            ts = ref.state[tp[i]]
            assert relerr(got[1], ts['exp_avg'].numpy()) < 2e-7 and relerr(got[2], ts['exp_avg_sq'].numpy()) < 2e-7, (k, i)
    assert rs['applied'] == 1002 and True in seen
    assert F32(2.0 / (2.0 + 1e-6)) < 1                                     # the exact-norm step was clipped, by the 1e-6


def run_skip(p_np, grads, **kw):
    """steps over `grads` (None = no step); a -0.0 is planted in a parameter after the first step"""
    ps, opt = make_opt(p_np, 1e-2, **kw)
    snaps = []
    for k, gs in enumerate(grads):
        if gs is not None:
            give(ps, gs)
            opt.step()
        if k == 0:
            opt.flat_param[7] = -0.0
        snaps.append(snapshot(opt))
    return opt, snaps


def test_a_poisoned_step_is_skipped_bit_for_bit_and_only_with_the_flag():
    rng = np.random.RandomState(13)
    p_np = make_params(rng)
    g1, g2, g3 = draw_grads(rng), draw_grads(rng), draw_grads(rng)
    g2[4].reshape(-1)[12345] = np.nan
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    ps, opt = make_opt(p_np, 1e-2, **kw)
    give(ps, g1); opt.step()
    opt.flat_param[7] = -0.0
    after1 = snapshot(opt)
    assert int(after1[0][7]) == -2 ** 31
    give(ps, g2); opt.step()
    assert same(snapshot(opt), after1)
    st = opt.guard_stats()
    assert (st['applied'], st['skipped'], st['skipped_in_row']) == (1, 1, 1) and math.isnan(st['grad_norm'])
    give(ps, g3); opt.step()
    st = opt.guard_stats()
    assert (st['applied'], st['skipped'], st['skipped_in_row']) == (2, 1, 0)
    _, clean = run_skip(p_np, [g1, g3], **kw)                              # the run that was given only gradients 1 and 3
    assert same(snapshot(opt), clean[1]) and same(after1, clean[0])
    sd = opt.state_dict()
    assert all(float(s['step']) == 2.0 for s in sd['state'].values())
    # without the flag the same input does poison the parameters
    opt2, snaps = run_skip(p_np, [g1, g2], max_grad_norm=1.0, ema_decay=0.9)
    assert not torch.isfinite(opt2.flat_param).all() and not torch.isfinite(opt2.flat_ema).all()
    assert opt2.guard_stats()['applied'] == 2 and opt2.guard_stats()['skipped'] == 0


def test_inactive_ranges_and_padding_never_move_and_the_norm_is_over_the_active_tensors():
    rng = np.random.RandomState(14)
    p_np = make_params(rng)
    ps, opt = make_opt(p_np, 1e-2, max_grad_norm=1.0, ema_decay=0.5)
    dead = (1, 4)
    opt.set_inactive([ps[i] for i in dead])
    still = torch.ones(opt.numel, dtype=torch.bool)
    for i, (q, o) in enumerate(zip(ps, opt.offsets)):
        if i not in dead:
            still[o:o + q.numel()] = False
    assert int(still.sum()) > sum(ps[i].numel() for i in dead)             # the padding is in it too
    before = [s[still] for s in snapshot(opt)]
    for _ in range(3):
        gs = draw_grads(rng)
        for i, (q, g) in enumerate(zip(ps, gs)):
            if i not in dead:
                q.grad.copy_(torch.from_numpy(g))
        opt.step()
        want = math.sqrt(G.grad_sumsq([g for i, g in enumerate(gs) if i not in dead]))
        assert abs(opt.guard_stats()['grad_norm'] - want) <= 1e-12 * want
    assert same([s[still] for s in snapshot(opt)], before)
    moved = snapshot(opt)[0][~still] != bits(torch.cat([torch.from_numpy(np.pad(x.reshape(-1), (0, -x.size % 4))) for x in p_np]).cuda())[~still]
    assert bool(moved.any())
    assert sorted(opt.state_dict()['state']) == [0, 2, 3, 5]


def test_ema_weights_swaps_in_the_averages_and_back_bit_for_bit():
    rng = np.random.RandomState(15)
    ps, opt = make_opt(make_params(rng), 1e-2, ema_decay=0.9)
    assert torch.equal(opt.flat_ema, opt.flat_param) and opt.flat_ema.data_ptr() != opt.flat_param.data_ptr()
    for _ in range(2):
        give(ps, draw_grads(rng)); opt.step()
    raw, ema = bits(opt.flat_param), bits(opt.flat_ema)
    assert not torch.equal(raw, ema)
    ptrs, v0 = [q.data_ptr() for q in ps], [q._version for q in ps]
    with opt.ema_weights():
        assert torch.equal(bits(opt.flat_param), ema) and [q.data_ptr() for q in ps] == ptrs
        assert all(q._version > v for q, v in zip(ps, v0))
        v1 = [q._version for q in ps]
        for q, o in zip(ps, opt.offsets):
            assert torch.equal(bits(q), ema[o:o + q.numel()].view(q.shape))
    assert torch.equal(bits(opt.flat_param), raw) and torch.equal(bits(opt.flat_ema), ema)
    assert all(q._version > v for q, v in zip(ps, v1))
    model = torch.nn.ParameterList(ps)
    sd = opt.ema_state_dict(model)
    assert sorted(sd) == sorted(model.state_dict())
    for k, q in model.named_parameters():
        o = opt.offsets[int(k)]
        assert torch.equal(bits(sd[k]), ema[o:o + q.numel()].view(q.shape)) and sd[k].data_ptr() != opt.flat_ema.data_ptr() + 4 * o
    with pytest.raises(_capi.DirHipError):
        with make_opt(make_params(rng), max_grad_norm=1.0)[1].ema_weights():
            pass


def test_state_dict_round_trip_continues_identically():
    rng = np.random.RandomState(16)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    p_np = make_params(rng)
    ps, opt = make_opt(p_np, **kw)
    for k in range(4):
        gs = draw_grads(rng)
        if k == 2:
            gs[0].reshape(-1)[0] = np.inf
        give(ps, gs); opt.step()
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups', 'guard', 'ema'} and all(float(s['step']) == 3.0 for s in sd['state'].values())
    ps2, opt2 = make_opt([q.detach().cpu().numpy() for q in ps], **kw)
    opt2.load_state_dict(sd)
    assert opt2.guard_stats() == dict(opt.guard_stats(), grad_norm=0.0, clip_coef=1.0)
    for _ in range(3):
        gs = draw_grads(rng)
        give(ps, gs); give(ps2, gs)
        opt.step(); opt2.step()
        assert same(snapshot(opt), snapshot(opt2)) and opt.guard_stats() == opt2.guard_stats()
    assert opt.guard_stats()['applied'] == 6 and opt.guard_stats()['skipped'] == 1
    # a torch.optim.AdamW state (no 'guard', no 'ema') still loads and continues
    tp = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p_np]
    ref = torch.optim.AdamW(tp, 1e-3)
    for t in tp:
        t.grad = torch.from_numpy(rng.normal(0, 1, t.shape).astype(F32))
    ref.step()
    ps3, opt3 = make_opt([t.detach().numpy() for t in tp], **kw)
    opt3.load_state_dict(ref.state_dict())
    st = opt3.guard_stats()
    assert (st['applied'], st['skipped'], st['clipped']) == (1, 0, 0)
