"""The convolution sweep's helper (tests/helpers/conv_cases.py) on the CPU: the descriptor list is the list the sweep is meant to run and obeys
dir_conv2d_forward's argument rules; its float64 reference agrees with oracle.nnops.conv2d and with a literal loop nest; a plain float32
convolution of the same operands stays inside the per-element bound at c = 1 on every descriptor of every kind; and the check rejects seven
single defects of the kind a tile, tap, slab or tail bug produces -- two of which the max-norm gates of the existing parity tests let through."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import relerr
from oracle import nnops as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import conv_cases as CC  # noqa: E402

SEED = 1234
_CACHE = {}


def prepared(case, kind):
    """operands, float64 reference and S of one descriptor, computed once and shared (read-only) by the tests of this module"""
    key = (case.name, kind)
    if key not in _CACHE:
        o = CC.make(case, kind, SEED)
        _CACHE[key] = (o,) + CC.reference(case, o, kind)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------ the list
@pytest.mark.parametrize('kind', CC.KINDS)
def test_descriptor_list_is_what_the_sweep_is_meant_to_run(kind):
    L = CC.cases(kind)
    assert L == CC.cases(kind)                                          # deterministic
    per = {c: sum(1 for d in L if d.cls == c) for c in CC.CLASSES}
    want = dict(CC.COUNTS, splitk=CC.COUNTS['splitk'] if kind in CC.HALF_KINDS else 0)
    assert per == want and 100 <= sum(want.values()) <= 150
    by = lambda cls: [d for d in L if d.cls == cls]      # noqa: E731
    assert {d.M for d in by('m_tails')} >= set(CC.M_TAIL_VALUES) | {7, 80}
    assert any((d.B, d.Ho, d.Wo) == (1, 257, 1) for d in by('m_tails')) and any((d.B, d.Ho, d.Wo) == (1, 1, 7) for d in by('m_tails'))
    assert any((d.B, d.Ho, d.Wo) == (1, 1, 1) for d in by('m_tails')) and any((d.B, d.Ho, d.Wo) == (5, 4, 4) for d in by('m_tails'))
    assert sorted(d.Cout for d in by('n_tails')) == sorted(CC.N_TAIL_VALUES)
    assert {d.nk(kind) for d in by('k_slabs') if d.kh * d.kw == 1} == set(CC.NK_VALUES) and any(d.kh == 3 and d.nk(kind) == 9 for d in by('k_slabs'))
    geo = by('geometry')
    assert {(d.kh, d.stride, d.pad) for d in geo if d.kh == d.kw} >= set(CC.GEOMETRY_KSP)
    assert {((d.kh, d.kw), d.pad) for d in geo} >= set(CC.GEOMETRY_KERNELS)
    assert any(d.stride == 2 and d.H % 2 and d.W % 2 for d in geo) and any(d.stride == 2 and d.H % 2 == 0 and d.W % 2 == 0 for d in geo)
    assert any((d.H, d.W, d.kh, d.pad) == (1, 1, 3, 1) for d in geo) and any((d.H, d.W, d.kh, d.pad) == (2, 2, 3, 1) for d in geo)
    halo = by('halo')
    assert all(d.kh == 3 and d.stride == 1 and d.pad == 1 for d in halo) and {d.W for d in halo} >= {8, 16, 32, 9, 12}
    assert {(d.B, d.H, d.W) for d in halo} >= {(1, 8, 8), (3, 8, 8)}                               # rows > Ho, fewer images than segments
    took = [d for d in halo if CC.patch_expected(d, 12)]
    assert len(took) >= 3 and any(256 % d.Wo == 0 and not CC.patch_expected(d, 12) and not CC.patch_expected(d, 13) for d in halo)   # Ho % rows != 0
    sl = by('slices')
    assert any(d.in_coff and d.in_cs > d.in_coff + d.Cin for d in sl) and any(d.out_coff and d.out_cs > d.out_coff + d.Cout for d in sl)
    assert any(d.residual and d.res_coff and d.res_cs > d.Cout for d in sl)
    assert any(d.out == 'f32' and d.out_coff % 4 for d in sl) and any(d.out == 'f32' and d.residual and d.res_coff % 4 for d in sl)
    ep = by('epilogue')
    assert {(d.scale, d.shift, d.relu, d.residual) for d in ep if not d.pre and not d.neg_scale and d.out == 'same'} == {
        (a, b, c, e) for a in (False, True) for b in (False, True) for c in (False, True) for e in (False, True)}
    assert any(d.neg_scale and d.relu for d in ep) and {d.pre for d in ep if d.pad > 0} >= {'relu', 'linear'} and any(d.out == 'f32' for d in ep)
    du = by('dual')
    assert any(d.stride2 == 2 and d.H2 == 2 * d.Ho - 1 for d in du) and any(d.stride2 == 2 and d.H2 == 2 * d.Ho for d in du)
    assert any(d.Cin2 != d.Cin for d in du) and any(d.Cout % 64 for d in du)
    sk = by('splitk')
    if kind in CC.HALF_KINDS:
        assert {d.splits for d in sk} == {2, 3, 16} and all(d.nk(kind) % d.splits for d in sk) and any(d.M % 128 and d.Cout % 128 for d in sk)
    # the argument rules of conv_forward (csrc/conv.hip), restated
    bk, epc = (32, 4) if kind in ('f32', 'f16x3', 'f16') else (64, 8)
    for d in L:
        assert d.B > 0 and d.H > 0 and d.W > 0 and d.Ho > 0 and d.Wo > 0 and d.stride > 0 and d.pad >= 0, d.name
        assert d.Cin > 0 and d.Cin % bk == 0 and d.kh * d.kw <= 32, d.name
        assert d.in_coff % epc == 0 and d.in_cs % epc == 0 and d.in_coff + d.Cin <= d.in_cs, d.name      # 16-byte aligned input slices
        assert d.out_coff + d.Cout <= d.out_cs and d.res_coff + d.Cout <= d.res_cs, d.name
        assert d.M <= 300 and d.Cout <= 264 and d.K <= 2304, d.name
        assert d.out in ('same', 'f32') and (d.pre in (None, 'relu', 'linear')), d.name
        if d.Cin2:
            assert d.Cin2 % bk == 0 and (d.H2 - 1) // d.stride2 + 1 == d.Ho and (d.W2 - 1) // d.stride2 + 1 == d.Wo and not d.pre, d.name
        if d.splits > 1:
            assert kind in CC.HALF_KINDS and d.out == 'same' and CC.vector_epilogue(d, kind) and d.splits <= min(16, d.nk(kind)), d.name


def test_every_expected_family_has_three_descriptors_that_can_reach_it():
    """the launcher rules the sweep's per-class tallies rest on, restated on the list itself (16-bit kinds)"""
    for kind in CC.HALF_KINDS:
        for cls in CC.classes(kind):
            L, want = CC.cases(kind, cls), CC.EXPECTED[cls]['16']
            vec = [d for d in L if CC.vector_epilogue(d, kind) and not d.Cin2 and d.splits == 1]
            if 'igemm_ring' in want:
                assert sum(1 for d in L if d.nk(kind) >= 3 and not d.pre) >= 3, cls
            if 'pipe' in want or 'pipe8' in want:
                assert len(vec) >= 3, cls
            if 'big' in want:
                assert sum(1 for d in vec if d.Cout > 128 and d.M > 128 and not d.pre) >= 3, cls
            if 'patch' in want:
                assert sum(1 for d in vec if CC.patch_expected(d, 12)) >= 3, cls
            if 'stream' in want:
                assert sum(1 for d in vec if d.kh * d.kw == 1 and d.stride == 1 and d.pad == 0 and d.Cout % 128 == 0 and d.out == 'same') >= 3, cls
            if 'as' in want:
                assert sum(1 for d in vec if d.W in (8, 16, 32) and d.Cout % 128 == 0 and (d.H * d.W) % 64 == 0 and d.out == 'same' and d.stride == 1
                           and ((d.kh, d.kw, d.pad) in ((3, 3, 1), (1, 1, 0)))) >= 3, cls


# ------------------------------------------------------------------------------------------------------------------------- the reference
def _plain(case):
    return not case.pre and not case.Cin2


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_reference_agrees_with_the_numpy_oracle_on_square_kernels(kind):
    n = 0
    for case in CC.cases(kind):
        if case.kh != case.kw or not _plain(case):
            continue
        o, ref, _ = prepared(case, kind)
        want = N.conv2d(o['x'].astype(np.float64), o['w'].astype(np.float64), None, case.stride, case.pad)
        if case.scale:
            want = want * o['scale'].astype(np.float64).reshape(1, -1, 1, 1)
        if case.shift:
            want = want + o['shift'].astype(np.float64).reshape(1, -1, 1, 1)
        if case.residual:
            want = want + o['res']
        if case.relu:
            want = np.maximum(want, 0)
        _, S = prepared(case, kind)[1:]
        assert np.all(np.abs(ref - want) <= 2.0 ** -48 * S), case.name           # two float64 summation orders
        n += 1
    assert n >= 90


def test_reference_agrees_with_a_literal_loop_nest_on_the_two_smallest_cases():
    kind = 'f32'
    L = sorted((c for c in CC.cases(kind) if _plain(c) and c.kh * c.kw > 1 and (c.stride > 1 or c.kh != c.kw)), key=lambda c: c.M * c.Cout * c.K)[:2]
    assert len(L) == 2
    for case in L:
        o, ref, S = prepared(case, kind)
        x, w = o['x'].astype(np.float64), o['w'].astype(np.float64)
        out = np.zeros((case.B, case.Cout, case.Ho, case.Wo))
        for b in range(case.B):
            for n in range(case.Cout):
                for oy in range(case.Ho):
                    for ox in range(case.Wo):
                        acc = 0.0
                        for ky in range(case.kh):
                            for kx in range(case.kw):
                                iy, ix = oy * case.stride - case.pad + ky, ox * case.stride - case.pad + kx
                                if 0 <= iy < case.H and 0 <= ix < case.W:
                                    acc += float(np.dot(x[b, :, iy, ix], w[n, :, ky, kx]))
                        v = acc * (float(o['scale'][n]) if case.scale else 1.0) + (float(o['shift'][n]) if case.shift else 0.0)
                        v += float(o['res'][b, n, oy, ox]) if case.residual else 0.0
                        out[b, n, oy, ox] = max(v, 0.0) if case.relu else v
        assert np.all(np.abs(out - ref) <= 2.0 ** -48 * S), case.name


def test_operands_have_the_scale_structure():
    case = [c for c in CC.cases('bf16') if c.name == 'n_tails-N264_k3'][0]
    o, ref, S = prepared(case, 'bf16')
    x, w = o['x'], o['w']
    assert 0.03 < float((x == 0).mean()) < 0.07 and 0.03 < float((w == 0).mean()) < 0.07
    assert np.array_equal(x, torch.from_numpy(x).bfloat16().float().numpy())                    # stored in the kind's type
    nz = np.abs(x[x != 0])
    assert nz.min() >= 0.5 * 2.0 ** -12 * (1 - 2.0 ** -8) and nz.max() <= 1.5 * 2.0 ** 12
    # every input channel weighs the same in every output: |x_c| |w_nc| does not depend on e_c
    t = np.abs(x).mean((0, 2, 3))[None, :] * np.abs(w).mean((2, 3))
    t = t / t.mean(1, keepdims=True)
    assert t.max() < 3.0 and t.min() > 0.2
    assert S.max() / S[S > 0].min() > 2.0 ** 16                                                   # while outputs span many octaves
    pre = [c for c in CC.cases('f16x3') if c.pre][0]
    op = CC.make(pre, 'f16x3', SEED)
    assert set(np.abs(op['ps'])) <= {0.5, 1.0, 2.0} and np.all(op['pb'] * 64 == np.round(op['pb'] * 64)) and np.abs(op['pb']).max() <= 2
    amax = np.abs(CC._activated(pre, op, 'f16x3')).max() * op['in_scale']
    assert 2.0 ** 14 <= amax < 2.0 ** 15


# ------------------------------------------------------------------------------------- the reference alone stays inside the bound at c = 1
@pytest.mark.parametrize('kind', CC.KINDS)
def test_plain_float32_convolution_passes_the_check_at_c_1(kind):
    worst = 0.0
    for case in CC.cases(kind):
        o, ref, S = prepared(case, kind)
        v = CC.float32_result(case, o, kind)
        r = CC.check(CC.to_buffer(case, kind, v), ref, S, case, kind, c=1.0)
        worst = max(worst, r)
        if case.out == 'same':                                   # the same values held to the fp32 form of the bound
            f32case = case._replace(out='f32')
            worst = max(worst, CC.check(CC.to_buffer(f32case, kind, v), ref, S, f32case, kind, c=1.0))
    print('%s: float32 CPU convolution, worst |got - ref| / (sqrt(K) 2^-24 S) = %.3f' % (kind, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the checker has teeth
DEFECTS = ('swap_channels', 'drop_border_tap', 'skip_last_slab', 'pad_is_activated_zero', 'zero_last_row', 'shift_of_previous_channel',
           'double_rounding')


def defective(case, o, kind, defect):
    """the clean float32 result with ONE defect -> output buffer, or None where the defect does not apply to the descriptor"""
    c = case
    bk = CC.BK[kind]
    if defect == 'swap_channels':                                # two input channels of one output channel trade weights
        n0, c0 = c.Cout // 2, 0
        c1 = int(np.argmax(np.abs(o['e_c'] - o['e_c'][c0])))
        w = o['w'].copy()
        w[n0, [c0, c1]] = w[n0, [c1, c0]]
        return CC.to_buffer(c, kind, CC.float32_result(c, dict(o, w=w), kind))
    if defect == 'drop_border_tap':                              # one tap (the one that reads the pixel itself) is lost at the border pixels only
        ty, tx = min(c.pad, c.kh - 1), min(c.pad, c.kw - 1)

        def conv(a, w, a2, w2):
            wd = w.copy()
            wd[:, :, ty, tx] = 0
            v, vd = CC._conv(a, w, c.stride, c.pad), CC._conv(a, wd, c.stride, c.pad)
            border = np.zeros((c.Ho, c.Wo), bool)
            border[[0, -1], :] = True
            border[:, [0, -1]] = True
            v = np.where(border[None, None], vd, v)
            return v + CC._conv(a2, w2, c.stride2, 0) if c.Cin2 else v
        return CC.to_buffer(c, kind, CC.float32_result(c, o, kind, conv))
    if defect == 'skip_last_slab':                               # the last K slab of the last 128-wide N tile is never accumulated
        n0 = 128 * ((c.Cout - 1) // 128)
        key = 'w2' if c.Cin2 else 'w'
        w = o[key].copy()
        w[n0:, -bk:, -1, -1] = 0
        return CC.to_buffer(c, kind, CC.float32_result(c, dict(o, **{key: w}), kind))
    if defect == 'pad_is_activated_zero':                        # padded pixels go through the pre-activation: act(pre_shift) instead of zero
        if not c.pre or c.pad == 0:
            return None
        p = c.pad
        big = c._replace(H=c.H + 2 * p, W=c.W + 2 * p, pad=0)
        return CC.to_buffer(c, kind, CC.float32_result(big, dict(o, x=np.pad(o['x'], ((0, 0), (0, 0), (p, p), (p, p)))), kind))
    if defect == 'zero_last_row':                                # the last row of the M tail is never written (zero-initialised accumulators stored)
        v = CC.float32_result(c, o, kind).copy()
        v[-1, :, -1, -1] = 0
        return CC.to_buffer(c, kind, v)
    if defect == 'shift_of_previous_channel':                    # the last channel takes shift[n - 1]
        if not c.shift or c.Cout < 2:
            return None
        sh = o['shift'].copy()
        sh[-1] = sh[-2]
        return CC.to_buffer(c, kind, CC.float32_result(c, dict(o, shift=sh), kind))
    if defect == 'double_rounding':                              # a 16-bit output rounded twice: to bf16 through f16 (to f16 through bf16)
        dt = c.out_dtype(kind)
        if dt == torch.float32:
            return None
        v = torch.from_numpy(CC.float32_result(c, o, kind))
        via = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
        return CC.to_buffer(c, kind, v.clamp(-65504.0, 65504.0).to(via).float().numpy())
    raise KeyError(defect)


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'f16s'])
@pytest.mark.parametrize('defect', DEFECTS)
def test_check_rejects_every_single_defect(defect, kind):
    """with the constants the GPU sweep runs with (CC.C), on every descriptor where the defect changes a bit of the output.  Double rounding moves
    an element by a whole ulp only where the fp32 value lies within half an f16 ulp of a bf16 tie -- closer to it, on some elements, than the
    accumulation bound lets the true value lie: there no per-element check can tell it from a correct rounding of a nearby sum, so that defect
    must be rejected wherever an element it moved sits more than 2 acc from the tie."""
    applied = 0
    for case in CC.cases(kind):
        o, ref, S = prepared(case, kind)
        buf = defective(case, o, kind, defect)
        if buf is None:
            continue
        v = CC.float32_result(case, o, kind)
        clean = CC.to_buffer(case, kind, v)
        if torch.equal(buf, clean):
            continue
        if defect == 'double_rounding':
            g, g0 = (t[..., case.out_coff:case.out_coff + case.Cout].double().numpy().transpose(0, 3, 1, 2) for t in (buf, clean))
            _, acc, _ = CC.bound(ref, S, case, kind)
            moved = (g != g0) & np.isfinite(g)
            if not (moved & (np.abs(v.astype(np.float64) - 0.5 * (g + g0)) > 2 * acc) & (np.abs(ref) < 3e4)).any() and np.isfinite(g).all():
                continue
        applied += 1
        with pytest.raises(AssertionError):
            CC.check(buf, ref, S, case, kind)
    floor = {'pad_is_activated_zero': 3, 'double_rounding': 0 if kind == 'f32' else 30}.get(defect, 80)
    assert applied >= floor, (defect, kind, applied)


def test_the_max_norm_gates_let_defects_through():
    """why the per-element form exists: conftest.relerr at the gates of the existing parity tests (1e-2 bf16, 1.5e-3 f16 storage) accepts several
    of the same defects, on descriptors where check() rejects them"""
    missed = set()
    for kind, gate in (('bf16', 1e-2), ('f16s', 1.5e-3)):
        for case in CC.cases(kind):
            if case.out != 'same' or np.abs(prepared(case, kind)[1]).max() > 6e4:
                continue
            o, ref, S = prepared(case, kind)
            clean = CC.to_buffer(case, kind, CC.float32_result(case, o, kind))
            for defect in DEFECTS:
                buf = defective(case, o, kind, defect)
                if buf is None or torch.equal(buf, clean) or defect in missed:
                    continue
                g = buf[..., case.out_coff:case.out_coff + case.Cout].float().numpy().transpose(0, 3, 1, 2)
                if relerr(g, ref) < gate:
                    with pytest.raises(AssertionError):
                        CC.check(buf, ref, S, case, kind)
                    missed.add(defect)
    print('defects the max-norm gates accept somewhere:', sorted(missed))
    assert len(missed) >= 2
