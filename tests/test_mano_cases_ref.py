"""CPU: the case lists, restatements, error scales, constants and mutants of tests/helpers/mano_cases.py -- everything the per-element gate of
the MANO kernels (tests/test_gpu_mano_sweep.py) rests on, checked without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import grad as OG
from oracle import gt_mano as G
from oracle import mano as OM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import mano_cases as M  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def measured():
    F, Ft, tol = M.measure_forward()
    return dict(forward=F, forward_root_operand=Ft, tol=tol, gt=M.measure_gt(), backward=M.measure_backward(np.load(os.path.join(GOLDEN, 'g13_mano_grad.npz'))))


def test_lists_are_what_the_docstring_says():
    fc, bc, gc = M.forward_cases(), M.backward_cases(), M.gt_cases()
    assert len(fc) == 105 and len(bc) == 33 and len(gc) == 40 and len(fc) + len(bc) + len(gc) < 400
    assert len({c.name for c in fc + bc}) == len(fc) + len(bc) and len({c.name for c in gc}) == len(gc)
    for cases in (fc, bc):
        assert {c.jc for c in cases} == set(M.JOINT_CLASSES) and {c.rc for c in cases} == set(M.ROOT_CLASSES)
        assert {c.side for c in cases} == {'left', 'right'} and {c.kind for c in cases} == {'pca', 'ident'}
        assert {c.center for c in cases} >= {-1, 0, 9} and {c.center for c in cases} & set(M.TIP_CENTRES)
        assert {float(c.para[61]) for c in cases} == {np.float32(s) for s in M.CAM_S}
        assert 10 * sum(c.rc == 'degenerate' for c in cases) <= len(cases)                     # the 10 % cap
        for c in cases:                                                                        # the exact joint classes are exact
            assert c.para.dtype == np.float32 and (c.kind == 'ident') == (c.jc in M.EXACT_JOINTS)
    assert {c.center for c in fc} >= set(M.TIP_CENTRES)
    assert {c.root_palm for c in fc} == {True, False} and not any(c.root_palm for c in bc)
    assert all(np.abs(c.para[:3]).max() > 0 and np.abs(c.para[3:6]).max() > 0 for c in bc)     # no exactly-zero 6D column in the backward list
    eps = [c for c in fc if c.jc == 'eps']
    assert all((c.para[6:51] == np.float32(-1e-8)).any() for c in eps) and all(set(np.abs(c.para[6:51]).tolist()) <= {float(np.float32(e)) for e in M.EPS_SET} for c in eps)
    for c in fc:
        n = np.linalg.norm(c.para[6:51].astype(np.float64).reshape(15, 3), axis=1)
        if c.jc == 'zero':
            assert (n == 0).all()
        elif c.jc == 'small':
            assert (np.abs(c.para[6:51]) >= 1e-4 * 0.999).all() and (np.abs(c.para[6:51]) <= 1e-2 * 1.001).all()
        elif c.jc in ('pi', 'twopi'):
            assert (np.abs(n / (np.pi * (1 if c.jc == 'pi' else 2)) - 1) < 2.0 ** -11).all()
        elif c.jc == 'large':
            assert (n >= 9.99).all() and (n <= 60.01).all()
        elif c.jc == 'one_hot':
            assert (n > 0).sum() == 1 and n.max() >= 10
    sub = [np.linalg.norm(c.para[:6].astype(np.float64).reshape(2, 3), axis=1).min() for c in fc if c.rc == 'sub_clamp']
    assert any(s < 0.6e-8 for s in sub) and any(1.9e-8 < s < 2.1e-8 for s in sub)
    assert {c.ncomps for c in gc} == {1, 7, 12, 45, 0} and {c.center for c in gc} >= {-1, 0, 9} and {c.center for c in gc} & set(M.TIP_CENTRES)
    assert {c.new_skel for c in gc} == {True, False} and {c.scale is None for c in gc} == {True, False} and {c.trans is None for c in gc} == {True, False}
    assert all(abs(np.linalg.norm(c.trans) - 0.7) < 1e-6 for c in gc if c.trans is not None)
    assert {c.jc for c in gc} == set(M.JOINT_CLASSES)
    # both candidate tip vertices appear with cotangents that tell them apart, on both sides
    for side in ('left', 'right'):
        c = next(c for c in bc if c.side == side)
        cot = M.cotangents(c)['verts']
        assert np.abs(cot[444] - cot[445]).min() >= 6.0


def test_restatement_agrees_with_the_oracles_in_float64():
    for c in M.forward_cases():
        if c.root_palm:
            continue
        p = c.para[None].astype(np.float64)
        v, j = OM.mano_forward(M.tables(c.kind, c.side), p[:, :51], p[:, 51:61], c.side, None if c.center < 0 else c.center)
        ref = M.forward_ref(c)
        with np.errstate(invalid='ignore'):
            for got, k in ((v[0], 'verts'), (j[0], 'joints'), (OM.projection_batch_xy(p[:, 61], p[:, 62:64], j)[0], 'joint_uv'),
                           (OM.projection_batch_xy(p[:, 61], p[:, 62:64], v)[0], 'mesh_uv')):
                scale = max(1.0, abs(float(c.para[61])))
                assert np.array_equal(np.isfinite(got), np.isfinite(ref[k])) and np.nanmax(np.abs(got - ref[k]), initial=0.0) <= 1e-13 * scale, (c.name, k)
    for c in M.gt_cases():
        b = M.tables(c.kind, c.side)
        T = {'hands_components': b['th_comps'], 'hands_mean': b['th_hands_mean'].reshape(45), 'J_regressor': b['th_J_regressor'], 'weights': b['th_weights'],
             'posedirs': b['th_posedirs'], 'v_template': b['th_v_template'].reshape(778, 3), 'shapedirs': b['th_shapedirs']}
        T = {k: v.astype(np.float64) for k, v in T.items()}
        n = lambda a: None if a is None else np.asarray(a, np.float64)[None]  # noqa: E731
        v, j = G.gt_mano_forward(T, n(c.root), n(c.pose), n(c.shape), n(c.trans), None if c.scale is None else np.asarray([c.scale], np.float64),
                                 None if c.center < 0 else c.center, c.ncomps > 0, c.new_skel)
        ref = M.gt_ref(c)
        assert np.abs(v[0] - ref['verts']).max() <= 1e-13 and np.abs(j[0] - ref['joints']).max() <= 1e-13, c.name


def test_autograd_agrees_with_central_differences_and_g13():
    """oracle/grad.py (h = 1e-6) is usable where the function is benign: normal root, joint classes small / normal, moderate cam scale"""
    n = 0
    for c in M.backward_cases():
        if c.rc != 'normal' or c.jc not in ('small', 'normal') or abs(float(c.para[61])) > 10:
            continue
        cot = M.cotangents(c)
        ref = OG.mano_vjp(M.tables(c.kind, c.side), c.para[None].astype(np.float64), c.side, None if c.center < 0 else c.center,
                          cot['verts'][None], cot['joints'][None], cot['joint_uv'][None], cot['mesh_uv'][None])[0]
        g = M.backward_ref(c)
        assert np.abs(g - ref).max() <= 1e-7 * np.abs(ref).max(), c.name                       # central differences: h^2 f''' / 6 + 2^-53 f / h
        n += 1
    assert n >= 4
    g13 = np.load(os.path.join(GOLDEN, 'g13_mano_grad.npz'))
    for c, pre, b in M.g13_cases():
        for sel, kinds in M.G13_SEL.items():
            ref = g13[pre + '.' + sel][b]
            assert np.abs(M.backward_ref(c, kinds) - ref).max() <= 1e-5 * np.abs(ref).max(), (c.name, sel)      # the golden is fp32 autograd


def test_float32_references_stay_inside_a_quarter_of_c_and_ratios_are_reproduced(measured):
    """RATIOS is recorded 5 % above the measurement: the re-measured ratio of every entry lies in (ratio / 1.5, ratio], i.e. both float32
    references are inside c / 4 everywhere.  S of the forward is a bound: a forward ratio above 1 would mean S misses a term."""
    for table in ('forward', 'forward_root_operand', 'gt', 'backward'):
        assert set(measured[table]) == set(M.RATIOS[table]), table
        for k, r in measured[table].items():
            assert M.RATIOS[table][k] / 1.5 < r <= M.RATIOS[table][k], (table, k, r, M.RATIOS[table][k])
    assert max(max(M.RATIOS[t].values()) for t in ('forward', 'forward_root_operand', 'gt')) < 1.0


def test_loose_tolerance_condition(measured):
    """on every element of a non-degenerate forward case the loose gate's tolerance stays below 2^-8 of the sample's max |verts| (the two
    projections: of max(1, |s|) max |verts|, their unit being s times a length); and the eps moved to `degenerate` do not meet it"""
    for k in M.KINDS:
        assert M.c_of('forward', k) * measured['tol'][k] < 2.0 ** -8, (k, measured['tol'][k])
    for c in M.forward_cases():
        if c.rc == 'degenerate' and ('near_parallel' in c.name or 'anti_parallel' in c.name):
            ref, S = M.forward_ref(c), M.forward_scale(c)
            vm = np.abs(ref['verts']).max()
            with np.errstate(invalid='ignore'):
                meets = [M.tolerance(ref[k], S[k], M.c_of('forward', k)).max() < 2.0 ** -8 * vm * (max(1.0, abs(float(c.para[61]))) if k.endswith('uv') else 1.0) for k in M.KINDS]
            assert not all(meets), c.name


def test_degenerate_flags_are_defined():
    for c in M.forward_cases():
        assert M.flag_f32(c) in (0, 1)
    assert sum(M.flag_f32(c) for c in M.nondegenerate(M.forward_cases())) == 0


@pytest.mark.parametrize('d', M.defects(), ids=[d.name for d in M.defects()])
def test_every_mutant_is_rejected(d):
    worst, old_ok = M.defect_report(d)
    print('%s: worst %.3g of the tolerance; the old max-norm gates on the benign cases %s it' % (d.name, worst, 'accept' if old_ok else 'reject'))
    if d.name in M.EQUIVALENT:
        assert worst <= 1.0 and old_ok          # no fp32 gate can see it (M.EQUIVALENT says why); if a case ever rejects it, move it out of that table
    else:
        assert worst > 1.0
    assert old_ok == (d.name in M.OLD_GATES_ACCEPT)
