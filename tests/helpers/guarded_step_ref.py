"""numpy restatement of the guarded AdamW step (include/dir_hip.h, "Guarded AdamW step") -- TEST INFRASTRUCTURE.

The norm is float64 (the sum of the float64 squares of the float32 gradients), everything else float32 in the kernel's operation order;
the update itself is oracle.optim.adamw_step.  Pinned against torch on the CPU (clip_grad_norm_ + torch.optim.AdamW + lerp_) and against
closed forms by tests/test_guarded_step_ref.py."""
import math

import numpy as np

from oracle.optim import adamw_step

F32 = np.float32


def grad_sumsq(grads):
    """float64 sum of squares over a list of float32 arrays"""
    return float(sum(np.sum(np.asarray(g, F32).astype(np.float64) ** 2) for g in grads))


def clip_coef(sumsq, max_norm):
    """(float)min(1.0, max_norm / (sqrt(sumsq) + 1e-6)); min(1.0, NaN) = 1.0"""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        c = np.float64(max_norm) / (np.sqrt(np.float64(sumsq)) + np.float64(1e-6))
    return F32(c) if c < 1.0 else F32(1.0)


def ema_update(e, p, decay):
    """torch's lerp_(p, w), w = (float)(1 - decay): e + w (p - e) for w < 0.5, p - (p - e)(1 - w) otherwise"""
    e, p = np.asarray(e, F32), np.asarray(p, F32)
    w = F32(1.0 - decay)
    d = (p - e).astype(F32)
    if w < F32(0.5):
        return (e + (w * d).astype(F32)).astype(F32)
    return (p - (d * (F32(1.0) - w)).astype(F32)).astype(F32)


def new_state():
    return {'applied': 0, 'skipped': 0, 'skipped_in_row': 0, 'clipped': 0, 'grad_norm': 0.0, 'clip_coef': F32(1.0), 'nonfinite': False}


def guarded_step(params, grads, ms, vs, emas, state, lr, max_norm=math.inf, skip_nonfinite=False, ema_decay=None, coef=None, **adam):
    """one step over lists of float32 arrays -> (params, ms, vs, emas); `state` (new_state()) is updated in place.  emas may be None.
    coef: use this coefficient for the update (the one a kernel published) instead of the restatement's own."""
    sumsq = grad_sumsq(grads)
    state['grad_norm'] = math.sqrt(sumsq) if sumsq >= 0 else float('nan')
    state['nonfinite'] = not math.isfinite(sumsq)
    state['clip_coef'] = clip_coef(sumsq, max_norm)
    if skip_nonfinite and state['nonfinite']:
        state['skipped'] += 1
        state['skipped_in_row'] += 1
        return params, ms, vs, emas
    state['applied'] += 1
    state['skipped_in_row'] = 0
    state['clipped'] += int(state['clip_coef'] < 1)
    c = state['clip_coef'] if coef is None else F32(coef)
    out_p, out_m, out_v, out_e = [], [], [], []
    for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        with np.errstate(invalid='ignore', over='ignore'):
            gs = (np.asarray(g, F32) * c).astype(F32)
            p2, m2, v2 = adamw_step(p, gs, m, v, state['applied'], lr, **adam)
        out_p.append(p2); out_m.append(m2); out_v.append(v2)
        if emas is not None and ema_decay is not None:
            out_e.append(ema_update(emas[i], p2, ema_decay))
    return out_p, out_m, out_v, (out_e if emas is not None and ema_decay is not None else emas)
