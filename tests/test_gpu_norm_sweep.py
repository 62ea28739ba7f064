"""The fp32 training operators of csrc/train_ops.hip at their dispatch edges and at hostile per-channel scales, element by element (cases, operands,
float64 references, S and the check: tests/helpers/norm_cases.py, proved on the CPU by tests/test_norm_cases_ref.py).  One test per class x variant:

 1. every case runs through the raw C ABI into canary-guarded buffers (strides ld > C, pointers 4 bytes off 16-byte alignment included): every
    output is held per element to |got - ref| <= c 2^-24 S against float64; guard floats, pad columns and the inputs must keep their bits;
 2. the launch log must name exactly the kernels the restated dispatch predicates expect for the case (a boundary case cannot pass by landing on
    the neighbouring path), and every kernel a class is meant to reach must serve at least three of its cases;
 3. every case runs a second time -- through dir_amd.train.ops where the case is contiguous and aligned -- and must give the same bits;
 4. where include/dir_hip.h promises the same bits they are asserted: dir_bn_train_stats (+ dir_bn_train_apply) against dir_bn_train_forward,
    dir_bn_train_stats_from_partials against dir_bn_train_forward_from_partials, attention with save_probs off against on.
SyncBN's building blocks run in ONE process on row splits of one batch, no collectives.

The constants c are NOT measured here: each is 4 x the larger error of two float32 CPU references (norm_cases.RATIOS), capped per case at the
serial bound (chain + 4).  For information, the kernels' own largest ratios on the MI355X, in units of 2^-24 S (NORM-CLASS lines of a -s run):

    kind        c      reference   kernel          kind        c      reference   kernel
    bn_mean     62.8      15.7       10.099         ln_gx       5.84e+05  1.46e+05   1.004
    bn_var      24.56     6.14       passed         ln_gw       4.88e+06  1.22e+06   1.669
    bn_rstd     19.68     4.92       3.832          ln_gb       22.24     5.56       3.993
    bn_running  32.2      8.05       4.753          att_probs   9.48      2.37       2.365
    bn_pre      10.24     2.56       1.071          att_out     5.92      1.48       1.474
    bn_y        62.8      15.7       10.058         att_gq      3.752     0.938      0.937
    bn_gx       10.52     2.63       1.670          att_gk      5.2       1.3        1.292
    bn_gw       7.48      1.87       1.351          att_gv      28.8      7.2        6.003
    bn_gb       13.64     3.41       2.426          gelu_y      20.88     5.22       2.163
    ln_mean     23.24     5.81       3.943          gelu_gx     15.12     3.78       1.315
    ln_rstd     185.2     46.3       1.982          colsum      67.2      16.8       7.087
    ln_y        10.52     2.63       1.660
(ln_gx / ln_gw are held to the serial cap C + 4 / R + 4, not to c; the SyncBN classes passed in a run that did not print their ratios.)  No kernel needed more than the references' own error allows; no guard float,
pad column or input was touched; every second run and every promised bit-equality held; no kernel defect was found.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from dir_amd import _capi
from dir_amd.train import ops as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import norm_cases as NC  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                                                            # canary floats before and after every buffer (a multiple of 4: alignment kept)
FILL, JUNK = NC.FILL, 30000.0                                         # outputs start as FILL; the pad columns of inputs hold JUNK
EPS, MOM = NC.EPS, NC.MOMENTUM


class Dev(object):
    """a [rows, cols] array at row stride ld inside a guarded device buffer, optionally 4 bytes off 16-byte alignment"""
    def __init__(self, rows, cols, ld=0, mis=False, src=None, fill=FILL):
        self.rows, self.cols, self.ld, self.is_vec = rows, cols, ld or cols, False
        self.off = GUARD + (1 if mis else 0)
        self.t = torch.full((2 * GUARD + 4 + rows * self.ld,), fill, device='cuda', dtype=torch.float32)
        if src is not None:
            self.view()[:, :cols] = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32).reshape(rows, cols)).cuda()
        self.t0 = self.t.clone()

    def view(self):
        return self.t[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)

    def ptr(self, row=0):
        return C.c_void_p(int(self.t.data_ptr() + 4 * (self.off + int(row) * self.ld)))

    def get(self):
        a = self.view()[:, :self.cols].cpu().numpy()
        return a.reshape(-1) if self.is_vec else a

    def tensor(self):
        """the contiguous tensor dir_amd.train.ops takes (contiguous, aligned arrays only)"""
        assert self.ld == self.cols and self.off == GUARD
        v = self.view()
        return v.reshape(-1) if self.is_vec else v

    def untouched(self):
        """guards and pad columns keep their bits"""
        chg = self.t.view(torch.int32) != self.t0.view(torch.int32)
        chg[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        return not bool(chg.any())

    def unchanged(self):
        return torch.equal(self.t.view(torch.int32), self.t0.view(torch.int32))


def vec(n, mis=False, src=None):
    d = Dev(1, n, mis=mis, src=src)
    d.is_vec = True
    return d


def P(d, row=0):
    return None if d is None else d.ptr(row)


class Log(object):
    """library calls with the kernels each launched (the launch log holds 32 names: reset per call)"""
    def __init__(self):
        self.names = []

    def __call__(self, name, *args):
        L = _capi.lib()
        L.dir_launch_log_reset()
        _capi.check(getattr(L, name)(*args), name)
        buf = C.create_string_buffer(2048)
        L.dir_launch_log_get(buf, 2048)
        self.names += [s for s in buf.value.decode().split(',') if s]


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def workspace(nbytes, mis=False):
    return vec(max(int(nbytes) // 4, 4), mis=mis)


# ===================================================================================================================== BatchNorm
class BnRun(object):
    """one BatchNorm case on the device through the raw C ABI"""
    def __init__(self, case, variant, o):
        self.case, self.variant, self.o = case, variant, o
        R, Cn, ld, mis = case.R, case.C, case.ld, case.mis
        self.x, self.gy = Dev(R, Cn, ld, mis, o['x'], JUNK), Dev(R, Cn, ld, mis, o['gy'], JUNK)
        self.res = Dev(R, Cn, ld, mis, o['res'], JUNK) if o['res'] is not None else None
        self.w = vec(Cn, mis, o['w']) if o['w'] is not None else None
        self.b = vec(Cn, mis, o['b']) if o['b'] is not None else None
        self.inputs = [d for d in (self.x, self.gy, self.res, self.w, self.b) if d is not None]
        self.relu, self.bwd = int(o['relu']), variant != 'relu_res'
        self.s = _capi.stream_ptr()

    def outputs(self):
        c = self.case
        R, Cn, ld, mis = c.R, c.C, c.ld, c.mis
        self.y, self.gx = Dev(R, Cn, ld, mis), (Dev(R, Cn, ld, mis) if self.o['need_gx'] and self.bwd else None)
        self.sm, self.sr, self.gw, self.gb = (vec(Cn, mis) for _ in range(4))
        self.rm, self.rv = vec(Cn, mis, self.o['rm0']), vec(Cn, mis, self.o['rv0'])
        self.outs = [d for d in (self.y, self.gx, self.sm, self.sr, self.gw, self.gb, self.rm, self.rv) if d is not None]

    def run(self):
        """-> (got, forward kernel names, backward kernel names, failures)"""
        self.outputs()
        got, fwd, bwd = getattr(self, 'run_' + self.case.api)()
        torch.cuda.synchronize()
        fails = ['%s: guard floats or pad columns of an output were written' % self.case.name for d in self.outs if not d.untouched()][:1]
        fails += ['%s: an input was written' % self.case.name for d in self.inputs if not d.unchanged()][:1]
        return got, fwd, bwd, fails

    def collect(self, **extra):
        got = dict(y=self.y.get(), mean=self.sm.get(), rstd=self.sr.get(), running_mean=self.rm.get(), running_var=self.rv.get())
        if self.bwd:
            got.update(gx=None if self.gx is None else self.gx.get(), gw=self.gw.get(), gb=self.gb.get())
        got.update(extra)
        return got

    def backward(self, log, entry='dir_bn_train_backward', ws_bytes=None):
        c = self.case
        n = _capi.lib().dir_bn_train_workspace_bytes(c.R, c.C) if ws_bytes is None else ws_bytes
        ws = workspace(n, c.mis) if n > 0 else None
        log(entry, P(self.gy), P(self.x), P(self.w), P(self.b), P(self.sm), P(self.sr), P(self.gx), P(self.gw), P(self.gb), c.R, c.C, c.ld, self.relu,
            P(ws), n, self.s)
        self.outs += [ws] if ws is not None else []

    def run_train(self):
        c, f, b = self.case, Log(), Log()
        n = _capi.lib().dir_bn_train_workspace_bytes(c.R, c.C)
        ws = workspace(n, c.mis) if n > 0 else None
        f('dir_bn_train_forward', P(self.x), P(self.w), P(self.b), P(self.y), P(self.sm), P(self.sr), P(self.rm), P(self.rv), c.R, c.C, c.ld, EPS, MOM,
          self.relu, P(self.res), P(ws), n, self.s)
        self.outs += [ws] if ws is not None else []
        if self.bwd:
            self.backward(b)
        return self.collect(), f.names, b.names

    def run_split(self):
        c, f, b = self.case, Log(), Log()
        n = _capi.lib().dir_bn_train_workspace_bytes(c.R, c.C)
        ws, ps, pb = workspace(n), vec(c.C), vec(c.C)
        f('dir_bn_train_stats', P(self.x), P(self.w), P(self.b), P(self.sm), P(self.sr), P(ps), P(pb), P(self.rm), P(self.rv), c.R, c.C, c.ld, EPS, MOM,
          P(ws), n, self.s)
        f('dir_bn_train_apply', P(self.x), P(self.w), P(self.b), P(self.sm), P(self.sr), P(self.y), c.R, c.C, c.ld, self.relu, P(self.res), self.s)
        # the same bits as dir_bn_train_forward: saved and running statistics, and stats + apply against forward
        y2, sm2, sr2, rm2, rv2 = Dev(c.R, c.C, c.ld), vec(c.C), vec(c.C), vec(c.C, src=self.o['rm0']), vec(c.C, src=self.o['rv0'])
        Log()('dir_bn_train_forward', P(self.x), P(self.w), P(self.b), P(y2), P(sm2), P(sr2), P(rm2), P(rv2), c.R, c.C, c.ld, EPS, MOM, self.relu,
              P(self.res), P(ws), n, self.s)
        self.same = all(same_bits(a.get(), d.get()) for a, d in ((self.y, y2), (self.sm, sm2), (self.sr, sr2), (self.rm, rm2), (self.rv, rv2)))
        self.outs += [ws, ps, pb]
        if self.bwd:
            self.backward(b)
        return self.collect(pre_scale=ps.get(), pre_shift=pb.get()), f.names, b.names

    def run_partials(self):
        c, o, f, b = self.case, self.o, Log(), Log()
        chunks = -(-c.R // c.chunk_rows)
        pad = np.full((c.cap - chunks, c.C), FILL, np.float32)
        mk = lambda a: Dev(c.cap, c.C, src=np.concatenate([a, pad]))      # noqa: E731
        p1, p2, q1, q2 = mk(o['p1']), mk(o['p2']), mk(o['p1']), mk(o['p2'])
        ps, pb, sm2, sr2, rm2, rv2 = vec(c.C), vec(c.C), vec(c.C), vec(c.C), vec(c.C, src=o['rm0']), vec(c.C, src=o['rv0'])
        f('dir_bn_train_forward_from_partials', P(self.x), P(p1), P(p2), c.chunk_rows, c.cap, P(self.w), P(self.b), P(self.y), P(self.sm), P(self.sr),
          P(self.rm), P(self.rv), c.R, c.C, c.ld, EPS, MOM, self.relu, P(self.res), self.s)
        Log()('dir_bn_train_stats_from_partials', P(q1), P(q2), c.chunk_rows, c.cap, P(self.w), P(self.b), P(sm2), P(sr2), P(ps), P(pb), P(rm2), P(rv2),
              c.R, c.C, EPS, MOM, self.s)
        self.same = all(same_bits(a.get(), d.get()) for a, d in ((self.sm, sm2), (self.sr, sr2), (self.rm, rm2), (self.rv, rv2)))
        self.outs += [ps, pb, p1, p2]
        if self.bwd:                                                  # backward partials by their documented meaning, float32 on the CPU
            torch.cuda.synchronize()
            mu, rs, y = self.sm.get(), self.sr.get(), self.y.get()
            g = np.where(y > 0, o['gy'], np.float32(0)) if self.relu else o['gy']
            xh = (o['x'] - mu) * rs
            st = np.arange(0, c.R, c.chunk_rows)
            bp1, bp2 = (Dev(chunks, c.C, src=np.add.reduceat(a, st, axis=0, dtype=np.float32)) for a in (g, g * xh))
            ws = workspace(2 * c.C * 4)
            b('dir_bn_train_backward_from_partials', P(self.gy), P(self.x), P(self.w), P(self.b), P(self.sm), P(self.sr), P(bp1), P(bp2), chunks,
              P(self.gx), P(self.gw), P(self.gb), c.R, c.C, c.ld, self.relu, P(ws), 2 * c.C * 4, self.s)
            self.inputs += [bp1, bp2]
        return self.collect(pre_scale=ps.get(), pre_shift=pb.get()), f.names, b.names

    def run_sync(self):
        c, f, b = self.case, Log(), Log()
        W, Cn = len(c.splits), c.C
        r0 = [0] + list(np.cumsum(c.splits))
        parts = Dev(W, 2 * Cn + 4, src=np.zeros((W, 2 * Cn + 4), np.float32))
        parts.view()[:, 2 * Cn] = torch.tensor(c.splits, dtype=torch.float32, device='cuda')
        for r, n in enumerate(c.splits):
            nb = _capi.lib().dir_bn_sync_workspace_bytes(n, Cn)
            f('dir_bn_sync_local_stats', P(self.x, r0[r]), parts.ptr(r), n, Cn, c.ld, P(workspace(nb)), nb, self.s)
        var = vec(Cn)
        f('dir_bn_sync_combine', P(parts), W, Cn, P(self.sm), P(var), P(self.rm), P(self.rv), MOM, self.s)
        mean = vec(Cn)                                                # the frozen forward copies the pooled mean into save_mean
        for r, n in enumerate(c.splits):
            f('dir_bn_frozen_forward', P(self.x, r0[r]), P(self.w), P(self.b), P(self.y, r0[r]), P(mean), P(self.sr), P(self.sm), P(var), n, Cn, c.ld, EPS,
              self.relu, P(self.res, r0[r]) if self.res is not None else None, self.s)
        self.outs += [var, mean]
        extra = dict(var=var.get())
        if self.bwd:
            sums = Dev(W, 2 * Cn)
            for r, n in enumerate(c.splits):
                nb = _capi.lib().dir_bn_sync_workspace_bytes(n, Cn)
                b('dir_bn_sync_backward_sums', P(self.gy, r0[r]), P(self.x, r0[r]), P(self.w), P(self.b), P(mean), P(self.sr), sums.ptr(r), n, Cn, c.ld,
                  self.relu, P(workspace(nb)), nb, self.s)
            pooled = vec(2 * Cn)
            pooled.view()[0] = sums.view().sum(0)                     # what the all-reduce does
            if self.gx is not None:
                for r, n in enumerate(c.splits):
                    b('dir_bn_sync_backward_apply', P(self.gy, r0[r]), P(self.x, r0[r]), P(self.w), P(self.b), P(mean), P(self.sr), P(pooled),
                      P(self.gx, r0[r]), n, float(c.R), Cn, c.ld, self.relu, self.s)
            self.outs += [sums]
            s = sums.get().reshape(W, 2 * Cn)
            extra.update(gb=s[:, :Cn].copy(), gw=s[:, Cn:].copy())
            self.same = same_bits(mean.get(), self.sm.get())
        got = self.collect()
        got.update(extra)
        return got, f.names, b.names

    def run_frozen(self):
        c, f, b = self.case, Log(), Log()
        f('dir_bn_frozen_forward', P(self.x), P(self.w), P(self.b), P(self.y), P(self.sm), P(self.sr), P(self.rm), P(self.rv), c.R, c.C, c.ld, EPS,
          self.relu, P(self.res), self.s)
        self.same = self.rm.unchanged() and self.rv.unchanged()       # the running statistics are inputs here
        if self.bwd:
            self.backward(b, 'dir_bn_frozen_backward', _capi.lib().dir_bn_frozen_workspace_bytes(c.R, c.C))
        got = self.collect()
        got['running_mean'] = got['running_var'] = None
        return got, f.names, b.names

    def run_ops(self):
        """the same case through dir_amd.train.ops (contiguous, aligned cases; SyncBN's wrappers need a process group) -> got, or None"""
        c, o = self.case, self.o
        if c.ld != c.C or c.mis or c.api == 'sync':
            return None
        T = lambda d: None if d is None else d.tensor()      # noqa: E731
        x, gy, w, b, res = T(self.x), T(self.gy), T(self.w), T(self.b), T(self.res)
        rm, rv = (torch.from_numpy(o[k].copy()).cuda() for k in ('rm0', 'rv0'))
        extra = {}
        if c.api == 'train':
            y, st = O.bn_train_fwd(x, w, b, rm, rv, EPS, MOM, relu=o['relu'], residual=res)
        elif c.api == 'split':
            st, pre = O.bn_train_stats(x, w, b, rm, rv, EPS, MOM)
            y = O.bn_train_apply(x, w, b, st, relu=o['relu'], residual=res)
            extra = dict(pre_scale=pre[0].cpu().numpy(), pre_shift=pre[1].cpu().numpy())
        elif c.api == 'partials':
            chunks = -(-c.R // c.chunk_rows)
            mk = lambda a: torch.from_numpy(np.concatenate([a, np.full((c.cap - chunks, c.C), FILL, np.float32)])).cuda()      # noqa: E731
            _, pre = O.bn_train_stats_from_partials((mk(o['p1']), mk(o['p2']), c.chunk_rows), c.R, w, b, rm.clone(), rv.clone(), EPS, MOM)
            y, st = O.bn_train_fwd_from_partials(x, (mk(o['p1']), mk(o['p2']), c.chunk_rows), w, b, rm, rv, EPS, MOM, relu=o['relu'], residual=res)
            extra = dict(pre_scale=pre[0].cpu().numpy(), pre_shift=pre[1].cpu().numpy())
        else:
            with O.frozen_batchnorm():
                y, st = O.bn_train_fwd(x, w, b, rm, rv, EPS, MOM, relu=o['relu'], residual=res)
        got = dict(y=y.cpu().numpy(), mean=st[0].cpu().numpy(), rstd=st[1].cpu().numpy(), running_mean=rm.cpu().numpy(), running_var=rv.cpu().numpy())
        if c.api == 'frozen':
            got['running_mean'] = got['running_var'] = None
        if self.bwd and c.api != 'partials' and not (o['relu'] and b is None):
            if c.api == 'frozen':
                with O.frozen_batchnorm():
                    gx, gw, gb = O.bn_train_bwd(gy, x, w, st, need_gx=o['need_gx'], b=b, relu=o['relu'])
            else:
                gx, gw, gb = O.bn_train_bwd(gy, x, w, st, need_gx=o['need_gx'], b=b, relu=o['relu'])
            got.update(gx=None if gx is None else gx.cpu().numpy(), gw=gw.cpu().numpy(), gb=gb.cpu().numpy())
        got.update(extra)
        return got


BN_PARAMS = [(cls, v) for cls in NC.BN_CLASSES for v in NC.BN_VARIANTS]


@pytest.mark.parametrize('cls,variant', BN_PARAMS, ids=['%s-%s' % p for p in BN_PARAMS])
def test_batchnorm_sweep(cls, variant):
    tally, failures, served = NC.Tally(), [], {}
    for case in NC.bn_cases(cls):
        o = NC.bn_make(case, variant)
        run = BnRun(case, variant, o)
        got, fwd, bwd, fails = run.run()
        failures += fails
        t = NC.bn_judge(case, variant, o, got)
        tally.merge(t)
        want_f, want_b = NC.bn_expected_kernels(case, variant)
        if fwd != want_f or bwd != (want_b if run.bwd else []):
            failures.append('%s/%s: launched %s | %s, expected %s | %s' % (case.name, variant, fwd, bwd, want_f, want_b if run.bwd else []))
        for k in set(fwd + bwd):
            served.setdefault(k, set()).add(case.name)
        if not getattr(run, 'same', True):
            failures.append('%s/%s: bits that include/dir_hip.h promises to be the same differ' % (case.name, variant))
        again = run.run_ops()
        how = 'through dir_amd.train.ops'
        if again is None:
            again, how = BnRun(case, variant, o).run()[0], 'again'
        diff = [k for k in again if k in got and not same_bits(again[k], got[k])]
        if diff:
            failures.append('%s/%s: run %s, %s differ in their bits' % (case.name, variant, how, diff))
    print('NORM-CLASS bn %s %s: %s; undecided band %.4f %%; cases per kernel %s' % (
        cls, variant, {k: '%.3f' % v[0] for k, v in sorted(tally.ratios.items())}, 100 * tally.band, {k: len(v) for k, v in sorted(served.items())}))
    for k in NC.bn_class_kernels(cls, variant):
        if len(served.get(k, ())) < 3:
            failures.append('%s %s: kernel %s served %d cases, at least 3 expected' % (cls, variant, k, len(served.get(k, ()))))
    failures += tally.failures
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:30]))


# ===================================================================================================================== LayerNorm
def ln_run(case, o, mode):
    R, Cn = case.R, case.C
    x, gy, w, b = Dev(R, Cn, src=o['x'], fill=JUNK), Dev(R, Cn, src=o['gy'], fill=JUNK), vec(Cn, src=o['w']), vec(Cn, src=o['b'])
    ax, awb = mode == 'accumulate_x', mode == 'accumulate_wb'
    y, mean, rstd = Dev(R, Cn), vec(R), vec(R)
    gx = None if mode == 'no_gx' else Dev(R, Cn, src=o['base_x'] if ax else None)
    gw, gb = vec(Cn, src=o['base_w'] if awb else None), vec(Cn, src=o['base_b'] if awb else None)
    log = Log()
    log('dir_layernorm_forward', P(x), P(w), P(b), P(y), P(mean), P(rstd), R, Cn, case.eps, _capi.stream_ptr())
    log('dir_layernorm_backward', P(gy), P(x), P(w), P(mean), P(rstd), P(gx), P(gw), P(gb), R, Cn, int(ax), int(awb), _capi.stream_ptr())
    torch.cuda.synchronize()
    ok = all(d.untouched() for d in (y, mean, rstd, gw, gb) + ((gx,) if gx is not None else ())) and all(d.unchanged() for d in (x, gy, w, b))
    got = dict(y=y.get(), mean=mean.get(), rstd=rstd.get(), gx=None if gx is None else gx.get(), gw=gw.get(), gb=gb.get())
    return got, log.names, ok


def ln_ops(case, o, mode):
    """the same through dir_amd.train.ops (its wrapper always forms g x)"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    x, gy, w, b = dev(o['x']), dev(o['gy']), dev(o['w']), dev(o['b'])
    y, st = O.layernorm_fwd(x, w, b, case.eps)
    ax, awb = mode == 'accumulate_x', mode == 'accumulate_wb'
    gx, gw, gb = O.layernorm_bwd(gy, x, w, st, gx=dev(o['base_x']) if ax else None, gw=dev(o['base_w']) if awb else None,
                                 gb=dev(o['base_b']) if awb else None, accumulate_x=ax, accumulate_wb=awb)
    return dict(y=y.cpu().numpy(), mean=st[0].cpu().numpy(), rstd=st[1].cpu().numpy(), gx=gx.cpu().numpy(), gw=gw.cpu().numpy(), gb=gb.cpu().numpy())


@pytest.mark.parametrize('mode', NC.LN_MODES)
def test_layernorm_sweep(mode):
    tally, failures = NC.Tally(), []
    for case in NC.ln_cases():
        o = NC.ln_make(case)
        got, names, ok = ln_run(case, o, mode)
        if not ok:
            failures.append('%s/%s: guard floats or an input were written' % (case.name, mode))
        want = ['layernorm_fwd_kernel'] + ([] if mode == 'no_gx' else ['layernorm_bwd_x_kernel']) + ['layernorm_bwd_wb_kernel']
        if names != want:
            failures.append('%s/%s: launched %s, expected %s' % (case.name, mode, names, want))
        tally.merge(NC.ln_judge(case, o, got, mode))
        again = ln_ops(case, o, mode)
        diff = [k for k in got if got[k] is not None and not same_bits(again[k], got[k])]
        if diff:
            failures.append('%s/%s: run through dir_amd.train.ops, %s differ in their bits' % (case.name, mode, diff))
    print('NORM-CLASS ln %s: %s' % (mode, {k: '%.3f' % v[0] for k, v in sorted(tally.ratios.items())}))
    failures += tally.failures
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:30]))


# ===================================================================================================================== attention
@pytest.mark.parametrize('kind', NC.ATT_KINDS)
def test_attention_sweep(kind):
    tally, failures = NC.Tally(), []
    s = _capi.stream_ptr()
    for case in [c for c in NC.att_cases() if c.kind == kind]:
        o = NC.att_make(case)
        B, T, H, D = case.B, case.T, case.H, NC.ATT_D
        qkv, gout = Dev(B * T, 3 * H * D, src=o['qkv'], fill=JUNK), Dev(B * T, H * D, src=o['gout'], fill=JUNK)
        probs, out, out2, gqkv = Dev(B * H * T, T), Dev(B * T, H * D), Dev(B * T, H * D), Dev(B * T, 3 * H * D)
        log = Log()
        log('dir_attention_forward', P(qkv), P(probs), P(out), B, T, H, o['scale'], s)
        log('dir_attention_backward', P(qkv), P(probs), P(gout), P(gqkv), B, T, H, o['scale'], s)
        log('dir_attention_forward', P(qkv), None, P(out2), B, T, H, o['scale'], s)                  # save_probs off: the same bits
        torch.cuda.synchronize()
        if log.names != ['attention_fwd_kernel', 'attention_bwd_kernel', 'attention_fwd_kernel']:
            failures.append('%s: launched %s' % (case.name, log.names))
        if not (all(d.untouched() for d in (probs, out, out2, gqkv)) and qkv.unchanged() and gout.unchanged()):
            failures.append('%s: guard floats or an input were written' % case.name)
        if not same_bits(out.get(), out2.get()):
            failures.append('%s: the output without probs differs from the output with probs' % case.name)
        got = dict(probs=probs.get().reshape(B, H, T, T), out=out.get(), gqkv=gqkv.get())
        tally.merge(NC.att_judge(case, o, got))
        o2, p2 = O.attention_fwd(qkv.tensor(), B, T, H, o['scale'])
        g2 = O.attention_bwd(qkv.tensor(), p2, gout.tensor(), B, T, H, o['scale'])
        if not (same_bits(o2.cpu().numpy(), got['out']) and same_bits(p2.cpu().numpy(), got['probs']) and same_bits(g2.cpu().numpy(), got['gqkv'])):
            failures.append('%s: run through dir_amd.train.ops, the bits differ' % case.name)
    print('NORM-CLASS attention %s: %s' % (kind, {k: '%.3f' % v[0] for k, v in sorted(tally.ratios.items())}))
    failures += tally.failures
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:30]))


# ===================================================================================================================== GELU, column sums
def test_gelu_sweep():
    tally, failures = NC.Tally(), []
    s = _capi.stream_ptr()
    for case in NC.gelu_cases():
        o = NC.gelu_make(case)
        n = len(o['x'])
        x, gy, y, gx = vec(n, src=o['x']), vec(n, src=o['gy']), vec(n), vec(n)
        log = Log()
        log('dir_gelu_forward', P(x), P(y), n, s)
        log('dir_gelu_backward', P(gy), P(x), P(gx), n, s)
        torch.cuda.synchronize()
        if log.names != ['gelu_fwd_kernel', 'gelu_bwd_kernel'] or not (y.untouched() and gx.untouched() and x.unchanged() and gy.unchanged()):
            failures.append('%s: launched %s, or guard floats / inputs were written' % (case.name, log.names))
        got = dict(y=y.get(), gx=gx.get())
        tally.merge(NC.gelu_judge(case, o, got))
        if not (same_bits(O.gelu_fwd(x.tensor()).cpu().numpy(), got['y']) and same_bits(O.gelu_bwd(gy.tensor(), x.tensor()).cpu().numpy(), got['gx'])):
            failures.append('%s: run through dir_amd.train.ops, the bits differ' % case.name)
    print('NORM-CLASS gelu: %s' % {k: '%.3f' % v[0] for k, v in sorted(tally.ratios.items())})
    failures += tally.failures
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:30]))


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
def test_colsum_sweep(accumulate):
    tally, failures, served = NC.Tally(), [], {}
    s = _capi.stream_ptr()
    for case in NC.colsum_cases():
        o = NC.colsum_make(case)
        x = Dev(case.R, case.N, case.ld, src=o['x'], fill=JUNK)
        nb = _capi.lib().dir_colsum_workspace_bytes(case.R, case.N)
        outs = []
        for _ in range(2):
            out, ws, log = vec(case.N, src=o['base'] if accumulate else None), (workspace(nb) if nb > 0 else None), Log()
            log('dir_colsum_f32', P(x), P(out), case.R, case.N, case.ld, int(accumulate), P(ws), nb, s)
            torch.cuda.synchronize()
            if not (out.untouched() and x.unchanged() and (ws is None or ws.untouched())):
                failures.append('%s: guard floats or the input were written' % case.name)
            outs.append(out.get())
        want = NC.colsum_expected_kernels(case, accumulate)
        if log.names != want:
            failures.append('%s: launched %s, expected %s' % (case.name, log.names, want))
        for k in log.names:
            served.setdefault(k, set()).add(case.name)
        tally.merge(NC.colsum_judge(case, o, outs[0], accumulate))
        again = O.colsum(x.tensor(), out=torch.from_numpy(o['base'].copy()).cuda() if accumulate else None, accumulate=accumulate) if case.ld == case.N else None
        if not same_bits(outs[0], outs[1]) or (again is not None and not same_bits(again.cpu().numpy(), outs[0])):
            failures.append('%s: a second run differs in its bits' % case.name)
    print('NORM-CLASS colsum %s: %s; cases per kernel %s' % (accumulate, {k: '%.3f' % v[0] for k, v in tally.ratios.items()}, {k: len(v) for k, v in served.items()}))
    failures += ['kernel %s served %d cases, at least 3 expected' % (k, len(v)) for k, v in served.items() if len(v) < 3]
    failures += tally.failures
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:30]))
