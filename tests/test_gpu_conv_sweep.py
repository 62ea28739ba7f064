"""The forward convolution kernels at edge descriptors, element by element (descriptors, operands, reference and check: tests/helpers/conv_cases.py,
proved on the CPU by tests/test_conv_cases_ref.py).  One test per descriptor class x kind; for every descriptor of the class

 1. dir_conv2d_forward with DIR_CONV_VARIANT 0 writes into a canary-filled buffer, held per element to |got - ref| <= acc + round_T(ref, acc),
    acc = c(kind) sqrt(K) 2^-24 S, against the float64 reference;
 2. every variant code the kind accepts must give the same bits, canaries included ("one accumulation order" is the library's contract);
 3. stride-1 1x1 descriptors also run dir_conv1x1_stream_forward (variants 0, 22, 23) and
 4. 16-bit stride-1 descriptors engine.ConvOp on the activation-stationary variants 25 .. 28, all bit for bit against step 1;
 5. dual-source descriptors (dir_conv2d_dual_forward / dual_scaled) are checked and compared across variants 0, 1, 4, 19;
 6. split-K descriptors are checked only (their summation order differs);
 7. the launch log says which kernel served each forced launch: a forced variant silently falls back to the four-wave kernel where it does not
    apply, so each class asserts that every kernel family it is meant to reach (conv_cases.EXPECTED) ran on at least three descriptors, that the
    halo-reuse kernel took exactly the descriptors patch_geometry accepts and that the ones it refuses were served by the pipelined or the
    four-wave kernel.  The log drops template arguments: the four-wave kernel counts as "on the ring" under variants 18 / 20 with nk >= 3 and no
    pre-activation (launch_conv's rule), the pipelined kernel as the eight-wave 128 x 64 form under variant 15.

c(kind): largest (|got - ref| - round_T) / (sqrt(K) 2^-24 S) over the whole list, measured on the MI355X with the check off
(DIR_CONV_SWEEP_MEASURE=1 makes step 1 measure and print instead of assert), times the project's margin of 4; check() caps it per descriptor at the
guaranteed (K + 2) 2^-24 S -- 2^-20 S for f16x3.

    kind     measured   c       worst descriptor (every fp32-output descriptor counts; 16-bit outputs after taking round_T off)
    f32      0.533      2.13    geometry-k3x1p0_9x11
    bf16     0.1085     0.434   m_tails-M65_1x5x13_k3 (16-bit products are exact in fp32: accumulation order alone)
    f16s     0.112      0.448   epilogue-f32_out_all
    f16x3    0.451      1.80    epilogue-pre_relu_k1p0 (with and without the pre-split pass: the same bits); closest to its 2^-20 S cap: halo-6x32,
                                K = 288, 0.258 of the 0.943 the cap allows
    f16      0.186      0.744   geometry-k1s2p0_8x10
No kind needs more than its cap, no variant, streaming or activation-stationary launch differed from variant 0 in a bit, no canary was touched.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from dir_amd import _capi
from dir_amd import engine as E
from dir_amd import functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import conv_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234
MEASURE = os.environ.get('DIR_CONV_SWEEP_MEASURE', '0') == '1'       # step 1 prints the ratios instead of asserting the bound
FILL = 3.0
JUNK = 30000.0                                                        # channels outside the input / residual slices
VARIANTS_16 = (1, 2, 3, 4, 17, 18, 20, 8, 9, 10, 11, 12, 13, 14, 15)
VARIANTS_F32 = (1, 2, 3, 4, 17, 18, 20)
VARIANTS_X = (1, 2, 3, 4, 17, 18, 20, 8, 9, 10, 11, 12, 13, 14, 15)  # test_training_convolution_variants_are_bit_identical's candidates
MODES = [('f32', False), ('bf16', False), ('f16s', False), ('f16x3', False), ('f16x3', True), ('f16', False), ('f16', True)]
PARAMS = [(cls, kind, pre) for kind, pre in MODES for cls in CC.classes(kind) if not (pre and cls == 'dual')]
KERNEL_FAMILY = {'conv_igemm_kernel': 'igemm', 'conv_pipe_kernel': 'pipe', 'conv_patch_kernel': 'patch', 'conv_big_kernel': 'big',
                 'stream1x1_kernel': 'stream', 'stream1x1p_kernel': 'stream', 'conv_as_kernel': 'as'}
_REF = {}


def prepared(case, kind):
    key = (case.name, kind)
    if key not in _REF:
        o = CC.make(case, kind, SEED)
        _REF[key] = (o,) + CC.reference(case, o, kind)
    return _REF[key]


def dev(a, dt=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt)


def nhwc_slice(a, dt, coff, cs):
    """NCHW numpy -> NHWC device buffer [B, H, W, cs] holding a at channels [coff, coff + C), JUNK elsewhere"""
    B, Cc, H, W = a.shape
    buf = torch.full((B, H, W, cs), JUNK, device='cuda', dtype=dt)
    buf[..., coff:coff + Cc] = dev(a.transpose(0, 2, 3, 1), dt)
    return buf


def launched():
    buf = C.create_string_buffer(1024)
    _capi.lib().dir_launch_log_get(buf, 1024)
    return buf.value.decode().split(',')


def family(names, case, kind, variant):
    fam = KERNEL_FAMILY.get(names[-1], names[-1])
    if fam == 'igemm' and variant in (18, 20) and case.nk(kind) >= 3 and not case.pre:
        return 'igemm_ring'
    if fam == 'pipe' and variant == 15:
        return 'pipe8'
    return fam


class Ops(object):
    """one descriptor's device operands and launchers"""
    def __init__(self, case, kind, presplit):
        self.c, self.kind, self.presplit = case, kind, presplit
        self.o, self.ref, self.S = prepared(case, kind)
        c, o, st = case, self.o, CC.STORE[kind]
        self.st, self.odt = st, case.out_dtype(kind)
        self.arith = kind if kind in ('f16x3', 'f16') else None
        self.x = nhwc_slice(o['x'], st, c.in_coff, c.in_cs)
        self.w = dev(o['w'].transpose(0, 2, 3, 1), st)
        self.scale, self.shift, self.ps, self.pb = dev(o['scale']), dev(o['shift']), dev(o['ps']), dev(o['pb'])
        self.res = nhwc_slice(o['res'], self.odt, c.res_coff, c.res_cs) if c.residual else None
        self.x2 = dev(o['x2'].transpose(0, 2, 3, 1), st) if c.Cin2 else None

    def out(self):
        c = self.c
        return torch.full((c.B, c.Ho, c.Wo, c.out_cs), FILL, device='cuda', dtype=self.odt)

    def conv(self, variant, splits=1):
        c = self.c
        out = self.out()
        _capi.lib().dir_launch_log_reset()
        F.conv2d_nhwc(self.x, self.w, c.stride, c.pad, self.scale, self.shift, relu=c.relu, residual=self.res, pre_scale=self.ps, pre_shift=self.pb,
                      pre_relu=c.pre == 'relu', out=out, out_coff=c.out_coff, in_coff=c.in_coff, cin=c.Cin, res_coff=c.res_coff, splits=splits,
                      arith=self.arith, variant=variant, presplit=self.presplit, in_scale=self.o['in_scale'])
        torch.cuda.synchronize()
        return out, launched()

    def dual(self, variant):
        c, L = self.c, _capi.lib()
        rows = torch.from_numpy(np.ascontiguousarray(CC.weight_rows(c, self.o))).cuda()
        code_in = {'f32': _capi.DT_F32, 'bf16': _capi.DT_BF16, 'f16s': _capi.DT_F16, 'f16x3': _capi.DT_F16X3, 'f16': _capi.DT_F16X1}[self.kind]
        code_out = {torch.float32: _capi.DT_F32, torch.bfloat16: _capi.DT_BF16, torch.float16: _capi.DT_F16}[self.odt]
        out = self.out()
        d = _capi.ConvDesc(c.B, c.H, c.W, c.Cin, c.in_cs, c.in_coff, c.Cout, c.out_cs, c.out_coff, 0, 0, 1, 1, 1, 0, code_in, code_out,
                           (1 if c.relu else 0) | (variant << 8), 0, 0, self.o['in_scale'] or 0.0)
        d2 = _capi.ConvSrc2(c.H2, c.W2, c.Cin2, c.Cin2, 0, c.stride2)
        L.dir_launch_log_reset()
        if self.arith:
            w, sc = F.pack_f16x3_weights(rows)
            sc = (sc / self.o['in_scale']).contiguous()
            rc = L.dir_conv2d_dual_scaled_forward(d, _capi.ptr(self.x), d2, _capi.ptr(self.x2), _capi.ptr(w), _capi.ptr(sc), _capi.ptr(self.shift),
                                                  _capi.ptr(out), _capi.stream_ptr())
        else:
            w = rows.to(self.st).contiguous()
            rc = L.dir_conv2d_dual_forward(d, _capi.ptr(self.x), d2, _capi.ptr(self.x2), _capi.ptr(w), _capi.ptr(self.shift), _capi.ptr(out),
                                           _capi.stream_ptr())
        _capi.check(rc, 'dual')
        torch.cuda.synchronize()
        return out, launched()

    def stream(self, variant):
        c = self.c
        out = self.out()
        _capi.lib().dir_launch_log_reset()
        F.conv1x1_stream(self.x, self.w.reshape(c.Cout, c.Cin), self.scale, self.shift, relu=c.relu, pre_scale=self.ps, pre_shift=self.pb,
                         pre_relu=c.pre == 'relu', out=out, out_coff=c.out_coff, in_coff=c.in_coff, cin=c.Cin, variant=variant)
        torch.cuda.synchronize()
        return out, launched()

    def conv_op(self):
        c = self.c
        return E.ConvOp(dev(self.o['w'], self.st), self.st, stride=1, pad=c.pad, scale=self.scale, shift=self.shift, relu=c.relu)

    def as_variant(self, op, variant):
        c = self.c
        out = self.out()
        E._TLS.variant = variant
        try:
            _capi.lib().dir_launch_log_reset()
            op(self.x, out=out, out_coff=c.out_coff, in_coff=c.in_coff, residual=self.res, res_coff=c.res_coff)
            torch.cuda.synchronize()
        finally:
            E._TLS.variant = None
        return out, launched()


def expected_halo_family(case, kind, variant):
    """DIR_CONV_VARIANT 12 .. 14 on a 16-bit kind: the halo-reuse kernel where patch_geometry accepts the descriptor; refused descriptors are served
    by the pipelined kernel of that tile, or by the four-wave kernel where that does not apply (scalar epilogue; a pre-activation on 256 x 128)"""
    if not CC.vector_epilogue(case, kind) or (case.pre and variant == 12):
        return 'igemm'
    return 'patch' if CC.patch_expected(case, variant) else 'pipe'


@pytest.mark.parametrize('cls,kind,presplit', PARAMS, ids=['%s-%s%s' % (c, k, '-presplit' if p else '') for c, k, p in PARAMS])
def test_conv_sweep(cls, kind, presplit):
    half = kind in CC.HALF_KINDS
    variants = VARIANTS_16 if half else VARIANTS_F32 if kind == 'f32' else VARIANTS_X
    failures, tally, worst, worst32 = [], {f: set() for f in CC.FAMILIES}, (0.0, ''), (0.0, '')
    for case in CC.cases(kind, cls):
        ops = Ops(case, kind, presplit)
        run = ops.dual if case.Cin2 else (lambda v: ops.conv(v, case.splits))
        base, names = run(0)
        tally.setdefault(family(names, case, kind, 0), set()).add(case.name)
        try:
            r = CC.check(base.cpu(), ops.ref, ops.S, case, kind, fill=FILL, enforce=not MEASURE)
        except AssertionError as e:
            failures.append(str(e))
            r = float('nan')
        if MEASURE:
            print('SWEEP-RATIO %s %s %s %.4f' % (kind + ('p' if presplit else ''), 'f32out' if ops.odt == torch.float32 else '16out', case.name, r))
        worst = max(worst, (r, case.name))
        if ops.odt == torch.float32:
            worst32 = max(worst32, (r, case.name))
        if case.splits > 1:
            continue
        for v in ((1, 4, 19) if case.Cin2 else variants):
            out, names = run(v)
            fam = family(names, case, kind, v)
            tally.setdefault(fam, set()).add(case.name)
            if not torch.equal(out, base):
                nd = int((out.view(torch.int16 if out.element_size() == 2 else torch.int32) != base.view(torch.int16 if out.element_size() == 2 else torch.int32)).sum())
                failures.append('%s [%s]: variant %d (%s) differs from variant 0 in %d elements' % (case.name, kind, v, ','.join(names), nd))
            if half and v in (12, 13, 14) and not case.Cin2 and fam != expected_halo_family(case, kind, v):
                failures.append('%s [%s]: variant %d ran %s, expected %s' % (case.name, kind, v, fam, expected_halo_family(case, kind, v)))
        plain = half and not case.Cin2 and case.out == 'same' and case.stride == 1
        if plain and case.kh * case.kw == 1 and case.pad == 0 and case.Cout % 128 == 0 and not case.residual:
            for v in (0, 22, 23):
                out, names = ops.stream(v)
                tally.setdefault(family(names, case, kind, v), set()).add(case.name)
                if not torch.equal(out, base):
                    d = (out.float() - base.float()).abs()
                    failures.append('%s [%s]: streaming kernel, variant %d, differs from the tiled kernel in %d elements (max %.3e)' % (
                        case.name, kind, v, int((d > 0).sum()), float(d.max())))
        if plain and not case.pre:
            d = _capi.ConvDesc(case.B, case.H, case.W, case.Cin, case.in_cs, case.in_coff, case.Cout, case.out_cs, case.out_coff,
                               case.res_cs if case.residual else 0, case.res_coff, case.kh, case.kw, 1, case.pad, E._dt(ops.st), E._dt(ops.st), 0, 0, 0, 1.0)
            sup = {v: bool(_capi.lib().dir_conv2d_as_supported(d, A, PB)) for v, (A, PB) in E.AS_VARIANTS.items()}
            if any(sup.values()):
                op = ops.conv_op()
                for v in E.AS_VARIANTS:
                    out, names = ops.as_variant(op, v)
                    if ('conv_as_kernel' in names) != sup[v]:
                        failures.append('%s [%s]: variant %d ran %s, dir_conv2d_as_supported says %s' % (case.name, kind, v, ','.join(names), sup[v]))
                    if sup[v]:
                        tally['as'].add(case.name)
                    if not torch.equal(out, base):
                        failures.append('%s [%s]: activation-stationary variant %d (%s) differs from the tiled kernel' % (case.name, kind, v, ','.join(names)))
    group = '16' if half else 'x' if presplit else '32'
    counts = {f: len(s) for f, s in tally.items()}
    print('SWEEP-CLASS %s %s%s: worst ratio %.4f (%s), worst on fp32 outputs %.4f (%s); descriptors per kernel family %s' % (
        cls, kind, 'p' if presplit else '', worst[0], worst[1], worst32[0], worst32[1], counts))
    for fam in CC.EXPECTED[cls][group]:
        if counts.get(fam, 0) < 3:
            failures.append('%s [%s]: kernel family %s ran on %d descriptors, at least 3 expected' % (cls, kind, fam, counts.get(fam, 0)))
    unknown = set(counts) - set(CC.FAMILIES)
    if unknown:
        failures.append('%s [%s]: unexpected kernels in the launch log: %s' % (cls, kind, sorted(unknown)))
    assert not failures, '%d failures:\n%s' % (len(failures), '\n'.join(failures[:40]))
