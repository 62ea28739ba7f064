"""dir_gemm_f32, dir_gemm_f32_grouped and dir_gemm_f32_splitk (csrc/train_ops.hip) at their tile tails, grid boundaries, strides and epilogues, element
by element (cases, operands, float64 references, S and the check: tests/helpers/matmul_cases.py, proved on the CPU by
tests/test_matmul_cases_ref.py).  One test per class x (trans_a, trans_b); for every case

 1. the raw C ABI writes C between two runs of 64 guard floats; guard floats, ldc pad columns and the floats between batch entries keep their bits,
    every input keeps its bits; a split-K workspace has exactly dir_gemm_f32_splitk_workspace_bytes bytes between 0xFF guard bytes;
 2. lda / ldb pad columns and the floats between batch entries and groups hold NaN: none may reach an output;
 3. every element is held to |got - ref64| <= min(c, terms + 2) 2^-24 S + 2^-149, S = sum |a b| + |bias| + |C0| of that element;
 4. the launch log names exactly the kernels the restated predicates expect, and every kernel serves at least three cases of its class;
 5. a second run gives the same bits.
The bit-identities include/dir_hip.h and train_ops.hip promise are tests of their own: 32 x 32 against 64 x 64 tiles (one product against `batch`
copies of it at stride_a = stride_b = 0), one group with batch == 1 against dir_gemm_f32 (M = 64, 65, 79, 80, 81: the 80-row tile too), reduce = 0
against one dir_gemm_f32 call per group.

c is NOT measured here (matmul_cases.RATIOS: 4 x the larger error of two float32 CPU references).  For information, the kernels' own largest
ratios on the MI355X in units of 2^-24 S (GEMM-CLASS lines of a -s run):

    kind      c       reference   kernel
    gemm      67.12   16.78       16.779 (grouped-M79_r1, trans_b: 9 groups of K = 33 in one accumulation; dir_gemm_f32 alone: 15.184, strides-big_plain)
    splitk    43.32   10.83       10.825 (splitk-K63, trans_b)
On their worst cases the kernels sit where the serial k-ascending float32 reference sits: the MFMA chain adds in that order.  Every case passed as
written: no guard float, pad column or input was touched, no NaN reached an output, every launch was the expected one, every second run and every
promised bit-identity held; no kernel defect was found.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from dir_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import matmul_cases as MC  # noqa: E402
import matmul_gpu_run as R  # noqa: E402

pytestmark = pytest.mark.gpu
PARAMS = [(cls, t) for cls in MC.GEMM_CLASSES for t in MC.TA_TB]


class GemmRun(object):
    """one case's device operands; run() -> (C as [batch, groups, M, N], kernel names, failures)"""
    def __init__(self, c, o):
        self.c, self.o, self.L = c, o, o['L']
        self.a, self.b = R.Buf(o['a'], c.mis & 1), R.Buf(o['b'], c.mis & 2)
        self.bias = R.Buf(o['bias']) if c.bias else None
        L = self.L
        self.d = _capi.GemmDesc(c.M, c.N, c.K, L.lda, L.ldb, L.ldc, c.ta, c.tb, int(c.acc), c.batch, L.sA, L.sB, L.sC)
        self.g = _capi.GemmGroups(c.ny, c.nx, c.reduce, 0, L.a_y, L.a_x, L.b_y, L.b_x, L.c_y, L.c_x)

    def run(self):
        c, L, lib = self.c, self.L, _capi.lib()
        out = R.Buf(self.o['c0'], c.mis & 4, guard=MC.FILL)
        args = (self.a.ptr(L.a0), self.b.ptr(L.b0), None if self.bias is None else self.bias.ptr(), out.ptr())
        fails, ws = [], None
        if c.api == 'gemm':
            _, names = R.call('dir_gemm_f32', C.byref(self.d), *args, _capi.stream_ptr())
        elif c.api == 'grouped':
            _, names = R.call('dir_gemm_f32_grouped', C.byref(self.d), C.byref(self.g), *args, _capi.stream_ptr())
        else:
            n = lib.dir_gemm_f32_splitk_workspace_bytes(C.byref(self.d))
            if n != -(-c.K // MC.GEMM_SPLIT_CHUNK) * c.M * c.N * 4:
                fails.append('%s: workspace of %d bytes, [chunks][M][N] floats expected' % (c.name, n))
            ws = R.Bytes(n)
            _, names = R.call('dir_gemm_f32_splitk', C.byref(self.d), *args, ws.ptr(), C.c_longlong(n), _capi.stream_ptr())
        torch.cuda.synchronize()
        if not out.untouched_outside(L.idxC):
            fails.append('%s: guard floats, ldc pad columns or the floats between batch entries of C were written' % c.name)
        if ws is not None and not ws.guards_intact():
            fails.append('%s: the guard bytes around the split-K workspace were written' % c.name)
        if not all(b.unchanged() for b in (self.a, self.b, self.bias) if b is not None):
            fails.append('%s: an input was written' % c.name)
        self.out = out
        return out.body()[torch.from_numpy(L.idxC).cuda()], names, fails


def sweep(cases, kind_of):
    failures, tally, worst = [], {}, {}
    for c in cases:
        o = MC.gemm_make(c)
        ref, S, terms = MC.gemm_reference(c, o)
        run = GemmRun(c, o)
        got, names, fails = run.run()
        failures += fails
        if names != MC.gemm_expected(c):
            failures.append('%s: launched %s, expected %s' % (c.name, names, MC.gemm_expected(c)))
        for k in names:
            tally[k] = tally.get(k, 0) + 1
        kind = kind_of(c)
        try:
            r = MC.check(got.cpu().numpy(), ref, S, kind, terms, c.name)
            worst[kind] = max(worst.get(kind, (0.0, '')), (r, c.name))
        except AssertionError as e:
            failures.append(str(e))
        again, _, _ = run.run()
        if not R.bits_equal(again, got):
            failures.append('%s: a second run gave other bits' % c.name)
    return failures, tally, worst


@pytest.mark.parametrize('cls,t', PARAMS, ids=['%s-t%d%d' % (cls, t[0], t[1]) for cls, t in PARAMS])
def test_gemm_sweep(cls, t):
    failures, tally, worst = sweep(MC.gemm_cases(cls, t), lambda c: 'splitk' if c.api == 'splitk' else 'gemm')
    print('GEMM-CLASS %s t%d%d: worst ratio per kind %s; cases per kernel %s' % (
        cls, t[0], t[1], {k: '%.3f (%s)' % v for k, v in worst.items()}, tally))
    for k in MC.GEMM_EXPECTED[cls]:
        if tally.get(k, 0) < 3:
            failures.append('%s: %s served %d cases, at least 3 expected' % (cls, k, tally.get(k, 0)))
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:40]))


def test_splitk_refuses_a_batch():
    c = MC.gemm_cases('splitk', (0, 0))[0]
    o = MC.gemm_make(c)
    run = GemmRun(c, o)
    run.d.batch = 2
    out, ws = R.Buf(o['c0'], guard=MC.FILL), R.Bytes(4 * c.M * c.N * 2)
    rc, names = R.call('dir_gemm_f32_splitk', C.byref(run.d), run.a.ptr(), run.b.ptr(), None, out.ptr(), ws.ptr(), C.c_longlong(ws.n), _capi.stream_ptr(),
                       expect_ok=False)
    torch.cuda.synchronize()
    assert rc != 0 and names == [] and out.unchanged() and bool((ws.t == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------------ promised bit-identities
def _plain(M, N, K, ta, tb, bias, acc):
    """the operands of one product: A, B, bias, the prefilled C"""
    rng = np.random.RandomState(M * 1000 + N * 10 + K + 2 * ta + tb)
    a, b = MC._vals(rng, M * K), MC._vals(rng, K * N)
    bz, c0 = (MC._vals(rng, N) if bias else None), MC._vals(rng, M * N)
    return a, b, bz, c0


@pytest.mark.parametrize('ta,tb', MC.TA_TB)
@pytest.mark.parametrize('bias,acc', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_small_and_large_tiles_give_the_same_bits(ta, tb, bias, acc):
    fails = []
    for M, N, K in ((65, 65, 37), (33, 129, 64), (127, 17, 97)):
        tiles = -(-M // 64) * -(-N // 64)
        batch = 128 // tiles + 1
        a, b, bz, c0 = _plain(M, N, K, ta, tb, bias, acc)
        A, B, Bz = R.Buf(a), R.Buf(b), (R.Buf(bz) if bias else None)
        lda, ldb = (M if ta else K), (K if tb else N)
        one, many = R.Buf(c0, guard=MC.FILL), R.Buf(np.tile(c0, batch), guard=MC.FILL)
        d1 = _capi.GemmDesc(M, N, K, lda, ldb, N, ta, tb, acc, 1, 0, 0, 0)
        dn = _capi.GemmDesc(M, N, K, lda, ldb, N, ta, tb, acc, batch, 0, 0, M * N)
        _, n1 = R.call('dir_gemm_f32', C.byref(d1), A.ptr(), B.ptr(), None if Bz is None else Bz.ptr(), one.ptr(), _capi.stream_ptr())
        _, nn = R.call('dir_gemm_f32', C.byref(dn), A.ptr(), B.ptr(), None if Bz is None else Bz.ptr(), many.ptr(), _capi.stream_ptr())
        torch.cuda.synchronize()
        assert n1 == ['gemm_f32_small_kernel'] and nn == ['gemm_f32_kernel'], (n1, nn)
        assert tiles <= 128 < tiles * batch
        for i in range(batch):
            if not torch.equal(many.body()[i * M * N:(i + 1) * M * N], one.body()):
                fails.append('M %d N %d K %d: copy %d on 64 x 64 tiles differs from the 32 x 32 product' % (M, N, K, i))
                break
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('ta', [0, 1])
def test_one_group_gives_the_bits_of_the_plain_gemm(ta):
    fails = []
    for i, M in enumerate((64, 65, 79, 80, 81)):
        N, K, tb, bias, acc = (33, 65, 129, 17, 64)[i], (37, 64, 5, 97, 33)[i], i % 2, i % 2, (i // 2) % 2
        a, b, bz, c0 = _plain(M, N, K, ta, tb, bias, acc)
        A, B, Bz = R.Buf(a), R.Buf(b), (R.Buf(bz) if bias else None)
        d = _capi.GemmDesc(M, N, K, (M if ta else K), (K if tb else N), N, ta, tb, acc, 1, 0, 0, 0)
        g = _capi.GemmGroups(1, 1, i % 2, 0, 0, 0, 0, 0, 0, 0)
        plain, grouped = R.Buf(c0, guard=MC.FILL), R.Buf(c0, guard=MC.FILL)
        R.call('dir_gemm_f32', C.byref(d), A.ptr(), B.ptr(), None if Bz is None else Bz.ptr(), plain.ptr(), _capi.stream_ptr())
        _, names = R.call('dir_gemm_f32_grouped', C.byref(d), C.byref(g), A.ptr(), B.ptr(), None if Bz is None else Bz.ptr(), grouped.ptr(), _capi.stream_ptr())
        torch.cuda.synchronize()
        assert names == ['gemm_f32_grouped_short_kernel' if 64 < M <= 80 else 'gemm_f32_grouped_kernel'], names
        if not torch.equal(plain.t, grouped.t):
            fails.append('M %d ta %d: one group differs from dir_gemm_f32 (%s)' % (M, ta, names[0]))
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('ta,tb', MC.TA_TB)
def test_side_by_side_groups_give_the_bits_of_one_gemm_each(ta, tb):
    fails = []
    for c in MC.gemm_cases('grouped', (ta, tb)):
        if c.reduce or c.ny * c.nx == 1:
            continue
        o = MC.gemm_make(c)
        run, L = GemmRun(c, o), o['L']
        got, _, _ = run.run()
        each = R.Buf(o['c0'], c.mis & 4, guard=MC.FILL)
        d = _capi.GemmDesc(c.M, c.N, c.K, L.lda, L.ldb, L.ldc, c.ta, c.tb, int(c.acc), 1, 0, 0, 0)
        for bz in range(c.batch):
            for g in range(c.ny * c.nx):
                gy, gx = divmod(g, c.nx)
                R.call('dir_gemm_f32', C.byref(d), run.a.ptr(L.a0 + bz * L.sA + gy * L.a_y + gx * L.a_x), run.b.ptr(L.b0 + bz * L.sB + gy * L.b_y + gx * L.b_x),
                       None if run.bias is None else run.bias.ptr(), each.ptr(bz * L.sC + gy * L.c_y + gx * L.c_x), _capi.stream_ptr())
        torch.cuda.synchronize()
        if not torch.equal(each.t, run.out.t):
            fails.append('%s: the grouped launch differs from one dir_gemm_f32 per group' % c.name)
    assert not fails, '\n'.join(fails)
