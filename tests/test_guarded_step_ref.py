"""CPU: the numpy restatement of the guarded AdamW step (tests/helpers/guarded_step_ref.py) against torch on the CPU
(clip_grad_norm_ + torch.optim.AdamW + lerp_) and against closed forms, and the host-side contract of the C ABI (no launch).

Tolerances: parameters and averages at the project's fp32 bound, 2e-7 (conftest.relerr; measured 1.3e-7 and 1.3e-7 over these 10 steps); the clipping
coefficient at 1e-5 relative (measured 2.5e-6: torch accumulates its norm in fp32, the restatement in float64)."""
import ctypes
import math
import os
import sys

import numpy as np
import torch

from conftest import relerr
from oracle import optim as OO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import guarded_step_ref as G  # noqa: E402

SHAPES = [(64, 3, 7, 7), (64,), (5, 3), (1,), (21, 128, 128), (1027,)]       # test_gpu_optim.py's
F32 = np.float32


def draw_grads(rng, small=False):
    """test_gpu_optim.py's gradient scales; small: a gradient whose global norm is below 1"""
    gs = [(rng.normal(0, 1, s) * 10.0 ** rng.randint(-4, 1)).astype(F32) for s in SHAPES]
    if small:
        n = math.sqrt(G.grad_sumsq(gs))
        gs = [(g * F32(0.25 / n)).astype(F32) for g in gs]
    return gs


def test_restatement_against_torch():
    rng = np.random.RandomState(1)
    decay, lr, max_norm = 0.9, 1e-3, 1.0
    tp = [torch.nn.Parameter(torch.from_numpy(rng.normal(0, 0.1, s).astype(F32))) for s in SHAPES]
    ref = torch.optim.AdamW(tp, lr)
    tema = [p.detach().clone() for p in tp]
    p = [t.detach().numpy().copy() for t in tp]
    m, v = [np.zeros(s, F32) for s in SHAPES], [np.zeros(s, F32) for s in SHAPES]
    e = [x.copy() for x in p]
    st = G.new_state()
    worst = {'p': 0.0, 'e': 0.0, 'coef': 0.0}
    for step in range(1, 11):
        gs = draw_grads(rng, small=step in (3, 6, 9))               # 3 steps whose norm is surely below max_norm
        for t, g in zip(tp, gs):
            t.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        tcoef = min(1.0, max_norm / (float(total) + 1e-6))
        ref.step()
        with torch.no_grad():
            for a, b in zip(tema, tp):
                a.lerp_(b.detach(), 1 - decay)
        p, m, v, e = G.guarded_step(p, gs, m, v, e, st, lr, max_norm=max_norm, ema_decay=decay)
        assert (st['clip_coef'] < 1) == (tcoef < 1), step
        assert step not in (3, 6, 9) or st['clip_coef'] == 1
        worst['coef'] = max(worst['coef'], abs(float(st['clip_coef']) - tcoef) / tcoef)
        for i in range(len(SHAPES)):
            worst['p'] = max(worst['p'], relerr(p[i], tp[i].detach().numpy()))
            worst['e'] = max(worst['e'], relerr(e[i], tema[i].numpy()))
    print('restatement vs torch: parameters %.3g, averages %.3g, coefficient %.3g' % (worst['p'], worst['e'], worst['coef']))
    assert st['applied'] == 10 and 4 <= st['clipped'] <= 7 and st['skipped'] == 0          # both branches occur
    assert worst['p'] < 2e-7 and worst['e'] < 2e-7 and worst['coef'] < 1e-5


def run_steps(n, **kw):
    rng = np.random.RandomState(5)
    p = [rng.normal(0, 0.1, s).astype(F32) for s in SHAPES]
    p0 = [x.copy() for x in p]
    m, v = [np.zeros(s, F32) for s in SHAPES], [np.zeros(s, F32) for s in SHAPES]
    e = [x.copy() for x in p]
    st = G.new_state()
    hist = []
    for _ in range(n):
        p, m, v, e = G.guarded_step(p, draw_grads(rng), m, v, e, st, 1e-2, **kw)
        hist.append((p, e))
    return p0, hist, st


def test_decay_zero_tracks_the_parameters_and_decay_one_keeps_the_start():
    p0, hist, _ = run_steps(5, max_norm=1.0, ema_decay=0.0)
    for p, e in hist:
        assert all(np.array_equal(a, b) for a, b in zip(p, e))
    p0, hist, _ = run_steps(5, max_norm=1.0, ema_decay=1.0)
    for p, e in hist:
        assert all(np.array_equal(a, b) for a, b in zip(p0, e)) and not any(np.array_equal(a, b) for a, b in zip(p0, p))


def test_a_skipped_step_changes_nothing_and_does_not_count():
    rng = np.random.RandomState(6)
    p = [rng.normal(0, 0.1, s).astype(F32) for s in SHAPES]
    m, v, e = [np.zeros(s, F32) for s in SHAPES], [np.zeros(s, F32) for s in SHAPES], [x.copy() for x in p]
    st = G.new_state()
    g1, g2, g3 = draw_grads(rng), draw_grads(rng), draw_grads(rng)
    for bad in (np.nan, np.inf, -np.inf):
        g2[5][-1] = bad
        assert not math.isfinite(G.grad_sumsq(g2))
    a = G.guarded_step(p, g1, m, v, e, st, 1e-2, max_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    b = G.guarded_step(a[0], g2, a[1], a[2], a[3], st, 1e-2, max_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    assert all(x is y for x, y in zip(a, b))                          # the very same arrays
    assert (st['applied'], st['skipped'], st['skipped_in_row'], st['nonfinite']) == (1, 1, 1, True)
    c = G.guarded_step(b[0], g3, b[1], b[2], b[3], st, 1e-2, max_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    assert (st['applied'], st['skipped'], st['skipped_in_row']) == (2, 1, 0)
    st2 = G.new_state()
    d = G.guarded_step(p, g1, m, v, e, st2, 1e-2, max_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    d = G.guarded_step(d[0], g3, d[1], d[2], d[3], st2, 1e-2, max_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    for x, y in zip(c, d):                                            # = the run that never saw the poisoned gradient
        assert all(np.array_equal(s, t) for s, t in zip(x, y))
    # without the flag the same gradient does poison the parameter it belongs to
    st3 = G.new_state()
    bad = G.guarded_step(a[0], g2, a[1], a[2], a[3], st3, 1e-2, max_norm=1.0, ema_decay=0.9)
    assert st3['applied'] == 1 and not np.isfinite(bad[0][5]).all()


def test_no_clipping_is_plain_adamw_bit_for_bit():
    rng = np.random.RandomState(7)
    p = [rng.normal(0, 0.1, s).astype(F32) for s in SHAPES]
    m, v = [np.zeros(s, F32) for s in SHAPES], [np.zeros(s, F32) for s in SHAPES]
    q, qm, qv = [x.copy() for x in p], [x.copy() for x in m], [x.copy() for x in v]
    st = G.new_state()
    for step in range(1, 8):
        gs = draw_grads(rng)
        p, m, v, _ = G.guarded_step(p, gs, m, v, None, st, 1e-3, max_norm=math.inf)
        assert st['clip_coef'] == 1 and st['clipped'] == 0
        for i, g in enumerate(gs):
            q[i], qm[i], qv[i] = OO.adamw_step(q[i], g, qm[i], qv[i], step, 1e-3)
            assert np.array_equal(p[i], q[i]) and np.array_equal(m[i], qm[i]) and np.array_equal(v[i], qv[i])


def test_coefficient_closed_forms():
    assert G.clip_coef(4.0, math.inf) == 1 and G.clip_coef(math.inf, math.inf) == 1 and G.clip_coef(math.nan, 1.0) == 1
    assert G.clip_coef(math.inf, 1.0) == 0
    assert G.clip_coef(4.0, 2.0) == F32(2.0 / (2.0 + 1e-6)) < 1      # norm == max_norm: clipped, by the 1e-6
    assert G.clip_coef(1e60, 1.0) == F32(1e-30)                       # a gradient of 1e30: its square overflows float, not double
    assert math.isfinite(G.grad_sumsq([np.array([1e30, 1.0], F32)]))


def test_guarded_entry_points_host_side_contract():
    """argument checks fail with a negative code and a message before anything touches a device; the workspace size is a pure function"""
    import torch  # noqa: F401,F811
    from dir_amd import _capi
    L = _capi.lib()
    ws = L.dir_grad_norm_workspace_bytes
    assert ws(0) == -1 and ws(-5) == -1
    sizes = [ws(n) for n in (1, 3, 4, 5, 1027, 1 << 20, 4 * 256 * 4096, 4 * 256 * 4096 + 7, 92_700_000, 1 << 33)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == 4096 * 8 and sizes[5] == 1024 * 8
    assert ctypes.sizeof(_capi.GuardState) == 80
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)

    def bad(rc, word):
        assert rc < 0 and word in L.dir_last_error(), (rc, L.dir_last_error())
    bad(L.dir_grad_guard(None, 16, 1.0, 0, 0.9, 0.999, one, 64, one, None), b'null pointer')
    bad(L.dir_grad_guard(one, 16, 1.0, 0, 0.9, 0.999, None, 64, one, None), b'null pointer')
    bad(L.dir_grad_guard(one, 16, 1.0, 0, 0.9, 0.999, one, 64, None, None), b'null pointer')
    bad(L.dir_grad_guard(one, 0, 1.0, 0, 0.9, 0.999, one, 64, one, None), b'n must be positive')
    bad(L.dir_grad_guard(odd, 16, 1.0, 0, 0.9, 0.999, one, 64, one, None), b'aligned')
    bad(L.dir_grad_guard(one, 16, 0.0, 0, 0.9, 0.999, one, 64, one, None), b'max_norm')
    bad(L.dir_grad_guard(one, 16, -1.0, 0, 0.9, 0.999, one, 64, one, None), b'max_norm')
    bad(L.dir_grad_guard(one, 16, math.nan, 0, 0.9, 0.999, one, 64, one, None), b'max_norm')
    bad(L.dir_grad_guard(one, 1 << 20, 1.0, 0, 0.9, 0.999, one, 64, one, None), b'workspace too small')
    args = (16, 1e-3, 0.9, 0.999, 1e-8, 1e-2)
    bad(L.dir_adamw_guarded_step(None, one, one, one, None, *args, 0.0, one, None), b'null pointer')
    bad(L.dir_adamw_guarded_step(one, one, one, None, None, *args, 0.0, one, None), b'null pointer')
    bad(L.dir_adamw_guarded_step(one, one, one, one, None, *args, 0.0, None, None), b'null pointer')
    bad(L.dir_adamw_guarded_step(one, one, one, one, None, 0, *args[1:], 0.0, one, None), b'n must be positive')
    bad(L.dir_adamw_guarded_step(one, odd, one, one, None, *args, 0.0, one, None), b'aligned')
    bad(L.dir_adamw_guarded_step(one, one, one, one, odd, *args, 0.5, one, None), b'aligned')
    bad(L.dir_adamw_guarded_step(one, one, one, one, one, *args, 1.5, one, None), b'ema_decay')
    bad(L.dir_adamw_guarded_step(one, one, one, one, one, *args, -0.1, one, None), b'ema_decay')
    bad(L.dir_adamw_guarded_step(one, one, one, one, one, *args, math.nan, one, None), b'ema_decay')
