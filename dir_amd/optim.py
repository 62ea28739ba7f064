"""Host-side mirror of the optimiser side of the reference's train.py, on libdir_hip.so.

  FlatAdamW            train.py:227   optim.AdamW([{'params': model.parameters(), 'initial_lr': lr}], lr): same defaults
                                       (betas (0.9, 0.999), eps 1e-8, weight_decay 0.01), same `state_dict()` layout, so a
                                       reference checkpoint's 'optimizer' entry loads and a saved one resumes under torch
  CosineAnnealingLR    train.py:229-230 optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max, eta_min=0) (closed form)
  MultiStepLR          train.py:231-232 optim.lr_scheduler.MultiStepLR(optimizer, [30], gamma=0.1) (torch's chained form)
  save_checkpoint / load_checkpoint    train.py:127-149  {'net', 'optimizer', 'schedule', 'last_epoch'}
                                       (+ 'ema' / 'guard' only when FlatAdamW's guard or average is on; the reference reads the four)
The parameters are moved into ONE contiguous fp32 buffer (each tensor becomes a view of it), gradients into a second one
(`.grad` of each parameter is a view), the two Adam moments are flat as well: `step()` is a single dir_adamw_step launch over
all of them, and `flat_grad` is the bucket a data-parallel all-reduce would reduce in one call.
The gradient views are filled by dir_amd.train (train/step.py::train_step, or `.backward()` on the losses of the mirror DIR in
training mode).
"""
import contextlib
import math

import torch

from . import _capi


class FlatAdamW(object):
    """max_grad_norm / skip_nonfinite / ema_decay (all unset: step() is the single dir_adamw_step launch per range, nothing else): the
    guarded step of include/dir_hip.h -- dir_grad_guard over the whole flat gradient (global norm in double, the clipping coefficient,
    the decision to skip a step whose gradient is not finite, AdamW's step count: all on the device), then dir_adamw_guarded_step per
    active range (clipped update, optional average).  step() reads nothing on the host.  It is called after average_gradients /
    bucketer.finish(), so every rank takes the norm of identical bytes and decides alike.  The average (`flat_ema`) starts as a copy of
    the parameters when it is switched on (timm's ModelEmaV2, not swa_utils' copy on the first update)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None):
        groups = list(params)
        if groups and isinstance(groups[0], dict):            # the reference passes one param group with 'initial_lr'
            assert len(groups) == 1, 'one parameter group (train.py:227)'
            self.extra = {k: v for k, v in groups[0].items() if k != 'params'}
            groups = list(groups[0]['params'])
        else:
            self.extra = {}
        self.params = [p for p in groups]
        assert self.params, 'no parameters'
        dev = self.params[0].device
        _capi.require_cuda(*self.params)
        for p in self.params:
            assert p.dtype == torch.float32 and p.device == dev
        # 16-byte aligned slots so that every view keeps vector alignment
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.numel = n
        self.flat_param = torch.zeros(n, device=dev)
        self.flat_grad = torch.zeros(n, device=dev)
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                self.flat_param[o:o + p.numel()].copy_(p.reshape(-1))
                p.data = self.flat_param[o:o + p.numel()].view(p.shape)
                p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.param_groups = [dict(self.defaults, **self.extra)]      # schedulers write param_groups[0]['lr']
        self.step_count = 0
        self.active = [True] * len(self.params)
        self._ranges = [(0, n)]
        self.max_grad_norm, self.skip_nonfinite, self.ema_decay = None, False, None
        self.flat_ema, self._guard_state, self._guard_ws = None, None, None
        if max_grad_norm is not None or skip_nonfinite or ema_decay is not None:
            self.configure(max_grad_norm, skip_nonfinite, ema_decay)

    # ---- the guarded step
    @property
    def guarded(self):
        return self._guard_state is not None

    def configure(self, max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        """switch the guarded step on (any argument set) or off (none): max_grad_norm > 0 (None = no clipping), skip_nonfinite,
        ema_decay in [0, 1] (None = no average).  Counters continue from `step_count`; the average starts as a copy of the parameters."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError('FlatAdamW: max_grad_norm must be positive, got %r' % (max_grad_norm,))
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError('FlatAdamW: ema_decay must be in [0, 1], got %r' % (ema_decay,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.max_grad_norm is None and not self.skip_nonfinite and self.ema_decay is None:
            if self.guarded:
                self.guard_stats()
            self.flat_ema, self._guard_state, self._guard_ws = None, None, None
            return
        dev = self.flat_param.device
        if not self.guarded:
            self._guard_state = torch.zeros(_capi.C.sizeof(_capi.GuardState), dtype=torch.uint8, device=dev)
            self._guard_ws = torch.zeros(_capi.lib().dir_grad_norm_workspace_bytes(self.numel) // 8, dtype=torch.float64, device=dev)
            self._write_guard(applied=self.step_count)
        if self.ema_decay is None:
            self.flat_ema = None
        elif self.flat_ema is None:
            self.flat_ema = self.flat_param.clone()

    def _write_guard(self, applied=0, skipped=0, skipped_in_row=0, clipped=0):
        st = _capi.GuardState(applied=int(applied), skipped=int(skipped), skipped_in_row=int(skipped_in_row), clipped=int(clipped), coef=1.0)
        self._guard_state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))

    def guard_stats(self):
        """ONE host read of the device's state: the norm and coefficient of the last step and the counters since the start of training"""
        if not self.guarded:
            raise _capi.DirHipError('FlatAdamW.guard_stats: the guarded step is off (max_grad_norm / skip_nonfinite / ema_decay)')
        st = _capi.GuardState.from_buffer_copy(self._guard_state.cpu().numpy().tobytes())
        self.step_count = st.applied
        return {'grad_norm': st.norm, 'clip_coef': st.coef, 'applied': st.applied, 'skipped': st.skipped,
                'skipped_in_row': st.skipped_in_row, 'clipped': st.clipped}

    def guard_settings(self):
        return {'max_grad_norm': self.max_grad_norm, 'skip_nonfinite': self.skip_nonfinite, 'ema_decay': self.ema_decay}

    def ema_state_dict(self, model):
        """model.state_dict() with every parameter replaced by its average (a copy); buffers -- BatchNorm running statistics, MANO tables --
        are the model's own"""
        if self.flat_ema is None:
            raise _capi.DirHipError('FlatAdamW.ema_state_dict: no average is kept (ema_decay is None)')
        index = {id(p): i for i, p in enumerate(self.params)}
        sd = model.state_dict()
        for k, p in model.named_parameters():
            i = index.get(id(p))
            if i is not None and k in sd:
                o = self.offsets[i]
                sd[k] = self.flat_ema[o:o + p.numel()].view(p.shape).clone()
        return sd

    @contextlib.contextmanager
    def ema_weights(self):
        """inside: the parameters ARE the averages (copied into flat_param on the device, version counters bumped so that DIR.engine()
        repacks); on exit the raw weights are back bit for bit.  Inactive slots and padding are equal in both stores."""
        if self.flat_ema is None:
            raise _capi.DirHipError('FlatAdamW.ema_weights: no average is kept (ema_decay is None)')
        raw = self.flat_param.clone()
        self.flat_param.copy_(self.flat_ema)
        torch._C._increment_version(self.params)
        try:
            yield self
        finally:
            self.flat_param.copy_(raw)
            torch._C._increment_version(self.params)

    def _guarded_step(self, g):
        L, s = _capi.lib(), _capi.stream_ptr()
        # the norm is taken over the WHOLE flat gradient: the padding between slots and the slots of inactive parameters are zero by
        # construction (allocated zeroed, zero_grad() zeroes in place, nothing writes a gradient there), so it is the norm over the
        # active tensors
        _capi.check(L.dir_grad_guard(_capi.ptr(self.flat_grad), self.numel, math.inf if self.max_grad_norm is None else self.max_grad_norm,
                                     int(self.skip_nonfinite), float(g['betas'][0]), float(g['betas'][1]), _capi.ptr(self._guard_ws),
                                     self._guard_ws.numel() * 8, _capi.ptr(self._guard_state), s), 'dir_grad_guard')
        for a, b in self._ranges:
            off = lambda t: None if t is None else _capi.C.c_void_p(t.data_ptr() + 4 * a)       # noqa: E731
            _capi.check(L.dir_adamw_guarded_step(off(self.flat_param), off(self.flat_grad), off(self.exp_avg), off(self.exp_avg_sq),
                                                 off(self.flat_ema), b - a, float(g['lr']), float(g['betas'][0]), float(g['betas'][1]),
                                                 float(g['eps']), float(g['weight_decay']), self.ema_decay or 0.0,
                                                 _capi.ptr(self._guard_state), s), 'dir_adamw_guarded_step')

    def set_inactive(self, params):
        """Parameters that never receive a gradient (torch.optim.AdamW skips `p.grad is None`: no state, no weight decay -- in the
        reference backbone.fc.* and interaction.STEblocks.0.*, never executed; NOT PGraphConv's e_0, whose gradient is a zero TENSOR there and
        which therefore decays -- dir_amd.train.step.inactive_parameters() is the authoritative list):
        step() leaves their slots alone and state_dict() omits them, as torch does."""
        ids = {id(p) for p in params}
        self.active = [a and id(p) not in ids for a, p in zip(self.active, self.params)]
        self._ranges, cur = [], None
        ends = self.offsets[1:] + [self.numel]
        for a, o, e in zip(self.active, self.offsets, ends):
            if a:
                cur = (cur[0], e) if cur is not None and cur[1] == o else (o, e)
                if self._ranges and self._ranges[-1][0] == cur[0]:
                    self._ranges[-1] = cur
                else:
                    self._ranges.append(cur)
            else:
                cur = None

    def zero_grad(self, set_to_none=False):
        # the gradients live in flat_grad (the all-reduce bucket): they are zeroed in place, never detached
        self.flat_grad.zero_()

    def step(self):
        g = self.param_groups[0]
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                raise _capi.DirHipError('FlatAdamW: a parameter\'s .grad no longer aliases flat_grad (zero_grad(set_to_none=True) on the '
                                        'model, or .grad reassigned): use FlatAdamW.zero_grad()')
        with torch.cuda.device(self.flat_param.device):
            if self.guarded:               # the device counts the applied steps; `step_count` follows at state_dict() / guard_stats()
                self._guarded_step(g)
            else:
                self.step_count += 1
                for a, b in self._ranges:
                    off = lambda t: _capi.C.c_void_p(t.data_ptr() + 4 * a)       # noqa: E731
                    _capi.check(_capi.lib().dir_adamw_step(off(self.flat_param), off(self.flat_grad), off(self.exp_avg), off(self.exp_avg_sq),
                                                           b - a, float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']),
                                                           float(g['weight_decay']), self.step_count, _capi.stream_ptr()), 'dir_adamw_step')
        # the kernel writes through raw pointers: bump every parameter's version counter as an in-place torch op would, so that
        # caches keyed on (data_ptr, _version) -- DIR.engine()'s packed weights -- see the update
        torch._C._increment_version(self.params)

    # ---- torch.optim.Optimizer.state_dict() layout: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [{..., 'params': [0..]}]}
    def state_dict(self):
        """guarded: 'step' is the device's count of APPLIED steps (one host read, at checkpoint time only)"""
        if self.guarded:
            self.guard_stats()
        state = {}
        if self.step_count > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                if not self.active[i]:
                    continue
                sl = slice(o, o + p.numel())
                state[i] = {'step': torch.tensor(float(self.step_count)), 'exp_avg': self.exp_avg[sl].view(p.shape).clone(),
                            'exp_avg_sq': self.exp_avg_sq[sl].view(p.shape).clone()}
        g = dict(self.param_groups[0])
        g.setdefault('amsgrad', False)
        g['params'] = list(range(len(self.params)))
        sd = {'state': state, 'param_groups': [g]}
        if self.guarded:                    # torch.optim.Optimizer.load_state_dict reads 'state' and 'param_groups' only
            sd['guard'] = self.guard_state_dict()
            if self.flat_ema is not None:
                sd['ema'] = self.flat_ema.clone()
        return sd

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        assert len(groups) == 1 and len(groups[0]['params']) == len(self.params), 'parameter count mismatch'
        g = {k: v for k, v in groups[0].items() if k != 'params'}
        g['betas'] = tuple(g['betas'])
        assert not g.get('amsgrad', False), 'amsgrad is not built'
        self.param_groups = [g]
        steps = set()
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            st = sd['state'].get(i, sd['state'].get(str(i)))
            if st is None:
                continue
            steps.add(int(float(st['step'])))
            sl = slice(o, o + p.numel())
            self.exp_avg[sl].copy_(st['exp_avg'].reshape(-1))
            self.exp_avg_sq[sl].copy_(st['exp_avg_sq'].reshape(-1))
        assert len(steps) <= 1, 'per-parameter step counts differ: not a state this optimiser can continue'
        self.step_count = steps.pop() if steps else 0
        if self.guarded:                    # a state without 'guard' (torch's, or one saved with the features off): the other counters start at 0
            gd = sd.get('guard', {})     # 'step' of the torch layout is the count of applied steps; the other counters ride in 'guard'
            self._write_guard(applied=self.step_count, **{k: gd.get(k, 0) for k in ('skipped', 'skipped_in_row', 'clipped')})
            if self.flat_ema is not None and 'ema' in sd:
                self.flat_ema.copy_(sd['ema'])

    def guard_state_dict(self):
        """the counters and settings (checkpoint key 'guard')"""
        st = self.guard_stats()
        return dict(self.guard_settings(), **{k: st[k] for k in ('applied', 'skipped', 'skipped_in_row', 'clipped')})

    def load_guard_state_dict(self, gd):
        if not self.guarded:
            raise _capi.DirHipError('FlatAdamW.load_guard_state_dict: the guarded step is off')
        self._write_guard(**{k: gd[k] for k in ('applied', 'skipped', 'skipped_in_row', 'clipped')})
        self.step_count = int(gd['applied'])

    def load_ema_state_dict(self, model, sd):
        """the averages of checkpoint key 'ema' (a state dict of `model`) into flat_ema"""
        if self.flat_ema is None:
            raise _capi.DirHipError('FlatAdamW.load_ema_state_dict: no average is kept (ema_decay is None)')
        index = {id(p): i for i, p in enumerate(self.params)}
        for k, p in model.named_parameters():
            i = index.get(id(p))
            if i is not None:
                o = self.offsets[i]
                self.flat_ema[o:o + p.numel()].copy_(sd[k].reshape(-1))


class CosineAnnealingLR(object):
    """optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max, eta_min) as train.py:229-230,84 uses it: step() once per epoch,
    lr = eta_min + (base_lr - eta_min) (1 + cos(pi epoch / T_max)) / 2 (torch's closed form)."""

    def __init__(self, optimizer, T_max, eta_min=0.0, last_epoch=-1):
        self.optimizer, self.T_max, self.eta_min = optimizer, T_max, eta_min
        self.base_lrs = [g.get('initial_lr', g['lr']) for g in optimizer.param_groups]
        for g, b in zip(optimizer.param_groups, self.base_lrs):
            g.setdefault('initial_lr', b)
        self.last_epoch = last_epoch
        self.step()

    def get_lr(self):
        return [self.eta_min + (b - self.eta_min) * (1 + math.cos(math.pi * self.last_epoch / self.T_max)) / 2 for b in self.base_lrs]

    def get_last_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g['lr'] = lr

    def state_dict(self):
        return {'T_max': self.T_max, 'eta_min': self.eta_min, 'base_lrs': list(self.base_lrs), 'last_epoch': self.last_epoch,
                '_step_count': self.last_epoch + 1, '_last_lr': self.get_last_lr()}

    def load_state_dict(self, sd):
        self.T_max, self.eta_min = sd['T_max'], sd['eta_min']
        self.base_lrs, self.last_epoch = list(sd['base_lrs']), sd['last_epoch']
        for g, lr in zip(self.optimizer.param_groups, sd.get('_last_lr', self.get_lr())):
            g['lr'] = lr


class MultiStepLR(object):
    """optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma) as train.py:231-232,84 uses it: step() once per epoch; when the epoch
    count reaches a milestone the current lr is multiplied by gamma (once per time the milestone is listed) -- torch's chained form, so the
    values are torch's to the bit.  state_dict() has torch's layout (milestones as a Counter)."""

    def __init__(self, optimizer, milestones, gamma=0.1, last_epoch=-1):
        from collections import Counter
        self.optimizer, self.milestones, self.gamma = optimizer, Counter(milestones), gamma
        self.base_lrs = [g.get('initial_lr', g['lr']) for g in optimizer.param_groups]
        for g, b in zip(optimizer.param_groups, self.base_lrs):
            g.setdefault('initial_lr', b)
        self.last_epoch = last_epoch
        self.step()

    def get_lr(self):
        n = self.milestones.get(self.last_epoch, 0)
        return [g['lr'] * self.gamma ** n if n else g['lr'] for g in self.optimizer.param_groups]

    def get_last_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g['lr'] = lr

    def state_dict(self):
        return {'milestones': self.milestones, 'gamma': self.gamma, 'base_lrs': list(self.base_lrs), 'last_epoch': self.last_epoch,
                '_step_count': self.last_epoch + 1, '_last_lr': self.get_last_lr()}

    def load_state_dict(self, sd):
        from collections import Counter
        self.milestones, self.gamma = Counter(sd['milestones']), sd['gamma']
        self.base_lrs, self.last_epoch = list(sd['base_lrs']), sd['last_epoch']
        for g, lr in zip(self.optimizer.param_groups, sd['_last_lr']):
            g['lr'] = lr


def save_checkpoint(path, model, optimizer, schedule, epoch):
    """train.py:137-149; + 'guard' (counters and settings) when the optimiser's guarded step is on, + 'ema' (the model's state dict with the
    averaged parameters: loads into DIR directly) when it keeps an average.  'net' stays the raw weights, which is what resuming needs."""
    ck = {'net': model.state_dict(), 'optimizer': optimizer.state_dict(), 'schedule': schedule.state_dict(), 'last_epoch': epoch}
    if 'guard' in ck['optimizer']:          # the file carries the two once, at its top level: 'optimizer' keeps torch's two keys
        ck['guard'] = ck['optimizer'].pop('guard')
        if ck['optimizer'].pop('ema', None) is not None:
            ck['ema'] = optimizer.ema_state_dict(model)
    torch.save(ck, path)


def load_checkpoint(path, model, optimizer, schedule):
    """train.py:127-135 -> start_epoch"""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    model.load_state_dict(ck['net'])
    optimizer.load_state_dict(ck['optimizer'])
    schedule.load_state_dict(ck['schedule'])
    if getattr(optimizer, 'guarded', False):
        # a checkpoint written without the features continues with fresh counters and an average that starts at its weights
        if 'guard' in ck:
            optimizer.load_guard_state_dict(ck['guard'])
        if optimizer.flat_ema is not None:
            optimizer.load_ema_state_dict(model, ck['ema'] if 'ema' in ck else ck['net'])
    return ck['last_epoch'] + 1
