"""dir_conv2d_wgrad_f32 (csrc/train_ops.hip) and dir_conv2d_wgrad_f16x3 / _pre (csrc/wgrad_x3.hip) at their dispatch edges, chunk plans, hostile
geometry and channel slices, element by element (cases, operands, float64 references, S and the check: tests/helpers/matmul_cases.py, proved on the
CPU by tests/test_matmul_cases_ref.py).  One test per class x variant; for every case

 1. the raw C ABI writes gw between two runs of 64 guard floats, which keep their bits, as does every input; the workspace has exactly the bytes
    the *_workspace_bytes function returns (the weight size for accumulate on one chunk) between 0xFF guard bytes and starts as 0xFF;
 2. the channels outside the in_coff / out_coff slices hold NaN: none may reach an output;
 3. every element is held to |got - ref64| <= c_eff 2^-24 S + 2^-149, S the sum of |gy x| over the in-image pixels of the element's tap (+ |gw0|):
    a tap wholly in the padding must be 0 to the last bit, with or without the fused pre-activation;
 4. the launch log names exactly the kernels the restated plan expects (fp32: kernel, chunk count and length restated and held against
    dir_conv2d_wgrad_workspace_bytes; f16x3: the chunk count is the device's, read from dir_conv2d_wgrad_f16x3_workspace_bytes and printed);
    every fp32 kernel, and every f16x3 tile shape x address form (by the restated predicates: the log drops template arguments), serves at
    least three cases of its class;
 5. a second run gives the same bits; the partial of an empty last chunk is all zeros;
 6. dir_conv2d_wgrad_f16x3_pre with pre_scale = 1, pre_shift = 0, pre_relu = 0 gives the bits of dir_conv2d_wgrad_f16x3 (the kernel's
    fmaf(v, 1, 0) is exact, and v x 0 masks padding pixels after it in both).

c is NOT measured here (matmul_cases.RATIOS).  For information, the kernels' own largest ratios on the MI355X in units of 2^-24 S and the f16x3
chunk counts seen there (WGRAD-CLASS lines of a -s run):

    kind      c_eff                 reference   kernel
    wgrad     min(39.1, terms + 2)  9.775       9.303 (slices-vector_both; accumulate: 9.061)
    x3        16 (the 2^-20 S cap)  16.93       9.456 (row4-128x128_260, relu; plain 8.853, lin 8.739; the CPU emulation of the split: 8.580)
f16x3 chunk counts on the MI355X: 1 for every case except chunked_32x32 4, chunked_32x32_k3 4, chunked_12x12 3, chunked_12x12_acc 3,
chunked_13x13 2, chunked_13x13_acc 2.  Every case passed as written: every tap wholly in the padding was 0 to the last bit (under the fused
pre-activation too), the empty 15th chunk's partial was all zeros, no guard was touched, no NaN reached an output, every launch was the expected
one, every second run and the identity pre-activation gave the same bits; no kernel defect was found.
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
F32_PARAMS = [(cls, v) for cls in MC.WGRAD_CLASSES for v in MC.WGRAD_VARIANTS]
X3_PARAMS = [(cls, v) for cls in MC.X3_CLASSES for v in MC.X3_VARIANTS]


class WgradRun(object):
    """one case's device operands; run() -> (gw [Cout, kh, kw, Cin], kernel names, chunk count, failures)"""
    def __init__(self, c, o):
        self.c, self.o = c, o
        self.x, self.gy = R.Buf(o['xbuf'], c.misx), R.Buf(o['gybuf'], c.misg)
        self.ps = R.Buf(o['ps']) if c.pre else None
        self.pb = R.Buf(o['pb']) if c.pre else None
        nat = ((c.H + 2 * c.pad - c.kh) // c.stride + 1, (c.W + 2 * c.pad - c.kw) // c.stride + 1)
        ho, wo = (0, 0) if nat == (c.Ho, c.Wo) else (c.Ho, c.Wo)                   # given in the descriptor only where it is not the natural size
        self.d = _capi.ConvDesc(c.B, c.H, c.W, c.Cin, c.in_cs if c.in_cs != c.Cin else 0, c.in_coff, c.Cout, c.out_cs if c.out_cs != c.Cout else 0,
                                c.out_coff, 0, 0, c.kh, c.kw, c.stride, c.pad, 0, 0, 0, ho, wo, 0.0, 0.0)
        self.n = c.Cout * c.kh * c.kw * c.Cin

    def run(self, identity_pre=None):
        c, o, lib, fails = self.c, self.o, _capi.lib(), []
        gw = R.Buf(o['gw0'] if c.acc else np.full(self.n, MC.FILL, np.float32), guard=MC.FILL)
        x3 = c.api == 'x3'
        nbytes = (lib.dir_conv2d_wgrad_f16x3_workspace_bytes if x3 else lib.dir_conv2d_wgrad_workspace_bytes)(C.byref(self.d))
        if nbytes % (4 * self.n) or nbytes == 4 * self.n:
            fails.append('%s: a workspace of %d bytes is no whole number (> 1) of partial gradients' % (c.name, nbytes))
        chunks = max(1, nbytes // (4 * self.n))
        if not x3 and nbytes != MC.wgrad_workspace_bytes(c):
            fails.append('%s: workspace of %d bytes, the restated plan says %d' % (c.name, nbytes, MC.wgrad_workspace_bytes(c)))
        if nbytes == 0 and c.acc:
            nbytes = 4 * self.n                                  # accumulate on one chunk: the weight size
        ws = R.Bytes(nbytes) if nbytes else None
        head = (C.byref(self.d), self.x.ptr(), self.gy.ptr(), gw.ptr(), int(c.acc), None if ws is None else ws.ptr(), C.c_longlong(nbytes))
        if not x3:
            _, names = R.call('dir_conv2d_wgrad_f32', *head, _capi.stream_ptr())
        elif identity_pre is not None:
            _, names = R.call('dir_conv2d_wgrad_f16x3_pre', *head, C.c_float(o['sx']), C.c_float(o['sg']), identity_pre[0].ptr(), identity_pre[1].ptr(), 0,
                              _capi.stream_ptr())
        elif c.pre:
            _, names = R.call('dir_conv2d_wgrad_f16x3_pre', *head, C.c_float(o['sx']), C.c_float(o['sg']), self.ps.ptr(), self.pb.ptr(),
                              int(c.pre == 'relu'), _capi.stream_ptr())
        else:
            _, names = R.call('dir_conv2d_wgrad_f16x3', *head, C.c_float(o['sx']), C.c_float(o['sg']), _capi.stream_ptr())
        torch.cuda.synchronize()
        if not gw.untouched_outside(np.arange(self.n)):
            fails.append('%s: guard floats around gw were written' % c.name)
        if ws is not None and not ws.guards_intact():
            fails.append('%s: the guard bytes around the workspace were written' % c.name)
        if not all(b.unchanged() for b in (self.x, self.gy, self.ps, self.pb) if b is not None):
            fails.append('%s: an input was written' % c.name)
        self.ws = ws
        return gw.body().view(c.Cout, c.kh, c.kw, c.Cin), names, chunks, fails


def sweep(cases):
    failures, tally, worst, chunk_counts = [], {}, (0.0, ''), []
    for c in cases:
        o = MC.wgrad_make(c)
        ref, S, terms = MC.wgrad_reference(c, o)
        run = WgradRun(c, o)
        got, names, chunks, fails = run.run()
        failures += fails
        if c.api == 'x3':
            want = ['conv_wgrad_x3_kernel'] + (['wgrad_x3_reduce_kernel'] if chunks > 1 or c.acc else [])
            tally[(MC.x3_tile(c), MC.x3_form(c))] = tally.get((MC.x3_tile(c), MC.x3_form(c)), 0) + 1
            chunk_counts.append('%s %d' % (c.name.split('-', 1)[1], chunks))
        else:
            want = MC.wgrad_expected(c)
            if chunks != MC.wgrad_plan(c)[1]:
                failures.append('%s: %d chunks, the restated plan says %d' % (c.name, chunks, MC.wgrad_plan(c)[1]))
            if c.name == 'chunks-empty_last_chunk' and not bool((run.ws.floats().view(chunks, -1)[-1].view(torch.int32) == 0).all()):
                failures.append('%s: the partial of the empty last chunk is not all zeros' % c.name)
        if names != want:
            failures.append('%s: launched %s, expected %s' % (c.name, names, want))
        for k in names:
            tally[k] = tally.get(k, 0) + 1
        try:
            worst = max(worst, (MC.check(got.cpu().numpy(), ref, S, 'x3' if c.api == 'x3' else 'wgrad', terms, c.name), c.name))
        except AssertionError as e:
            failures.append(str(e))
        again, _, _, _ = run.run()
        if not R.bits_equal(again, got):
            failures.append('%s: a second run gave other bits' % c.name)
    return failures, tally, worst, chunk_counts


@pytest.mark.parametrize('cls,variant', F32_PARAMS, ids=['%s-%s' % p for p in F32_PARAMS])
def test_wgrad_f32_sweep(cls, variant):
    failures, tally, worst, _ = sweep(MC.wgrad_cases(cls, variant))
    print('WGRAD-CLASS f32 %s %s: worst ratio %.3f (%s); cases per kernel %s' % (cls, variant, worst[0], worst[1], tally))
    for k in MC.WGRAD_EXPECTED[cls]:
        if tally.get(k, 0) < 3:
            failures.append('%s: %s served %d cases, at least 3 expected' % (cls, k, tally.get(k, 0)))
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:40]))


@pytest.mark.parametrize('cls,variant', X3_PARAMS, ids=['%s-%s' % p for p in X3_PARAMS])
def test_wgrad_f16x3_sweep(cls, variant):
    failures, tally, worst, chunk_counts = sweep(MC.x3_cases(cls, variant))
    print('WGRAD-CLASS x3 %s %s: worst ratio %.3f (%s); cases per kernel / (tile, form) %s; chunks: %s' % (
        cls, variant, worst[0], worst[1], {str(k): v for k, v in tally.items()}, ', '.join(chunk_counts)))
    if cls in MC.X3_FORMS:
        for tile in MC.X3_TILES:
            if tally.get((tile, MC.X3_FORMS[cls]), 0) < 3:
                failures.append('%s: tile %s in form %d served %d cases, at least 3 expected' % (cls, tile, MC.X3_FORMS[cls], tally.get((tile, MC.X3_FORMS[cls]), 0)))
        if not any(int(s.rsplit(' ', 1)[1]) > 1 for s in chunk_counts):
            failures.append('%s: the device split no case into several chunks' % cls)
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:40]))


@pytest.mark.parametrize('cls', MC.X3_CLASSES)
def test_identity_pre_activation_gives_the_bits_of_the_plain_gradient(cls):
    fails = []
    for c in MC.x3_cases(cls, 'plain'):
        o = MC.wgrad_make(c)
        run = WgradRun(c, o)
        plain, _, _, _ = run.run()
        one, zero = R.Buf(np.ones(c.Cin, np.float32)), R.Buf(np.zeros(c.Cin, np.float32))
        pre, names, _, f = run.run(identity_pre=(one, zero))
        fails += f
        if names[0] != 'conv_wgrad_x3_kernel' or not torch.equal(pre, plain):
            fails.append('%s: pre_scale 1, pre_shift 0 differs from dir_conv2d_wgrad_f16x3 (%s)' % (c.name, names))
    assert not fails, '\n'.join(fails)
