"""CPU: the case lists, restatements, error scales, constants and defects of tests/helpers/loss_cases.py -- everything the per-element gate of
the loss kernels (tests/test_gpu_loss_sweep.py) rests on, checked without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import losses as OL

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import loss_cases as L  # noqa: E402


@pytest.fixture(scope='module')
def measured():
    n = torch.get_num_threads()
    torch.set_num_threads(1)                     # float32 reductions move with the thread count
    try:
        r = dict(L.measure_dense())
        r.update(L.measure_stage())
    finally:
        torch.set_num_threads(n)
    return r


def test_lists_are_what_the_docstring_says():
    dc, sc = L.dense_cases(), L.stage_cases()
    assert len({c.name for c in dc}) == len(dc) and len({c.name for c in sc}) == len(sc)
    assert [(c.B, c.S) for c in dc[:15]] == list(L.DENSE_SIZES)
    assert sorted({c.B * c.S * c.S for c in dc[:15]}) == [1, 3, 225, 256, 289, 2023, 2048, 2064, 2116, 8100, 8192, 8281, 16384, 16562, 16640]
    assert max(c.B * c.S * c.S for c in dc) == 16640
    assert {c.labels for c in dc} == set(L.DENSE_LABELS) and {c.logits for c in dc} == set(L.DENSE_LOGITS)
    assert {c.class_weight for c in dc} == set(L.DENSE_CW) and {c.dense_weight for c in dc} == {1.0, 0.37} and {c.gout for c in dc} == set(L.DENSE_GOUT)
    hw = {(c.H, c.W) for c in dc}
    assert hw >= {(256, 256), (100, 100), (37, 37), (8, 8), (1, 1), (96, 64), (37, 100)} and any(c.H == c.S == c.W for c in dc)
    assert any((c.H, c.W, c.S) == (100, 100, 16) for c in dc) and any((c.H, c.W, c.S) == (37, 37, 20) for c in dc)       # the ratios 100 -> 16 and 37 -> 20
    assert any(c.H < c.S for c in dc) and any(c.H != c.W for c in dc) and any((c.S, c.H) == (32, 256) for c in dc) and any((c.S, c.H) == (4, 1) for c in dc)
    zero_present = 0
    for c in dc:                                                             # a zero class weight only where another class is present, labels as named
        seg, dense, gt_seg, gt_dense = L.dense_inputs(c)
        lab = OL.interpolate_nearest(gt_seg, c.S).astype(np.int64)
        present = set(np.unique(lab).tolist())
        assert sum(c.class_weight[k] for k in present) > 0, c.name
        zero_present += any(c.class_weight[k] == 0 for k in present)
        want = {'all': {0, 1, 2}, 'absent1': {0, 2}, 'only2': {2}}.get(c.labels, {0, 1})
        assert present <= want and (present == want or min(c.B * c.H * c.W, c.B * c.S * c.S) < 64), c.name
        assert seg.dtype == dense.dtype == gt_seg.dtype == gt_dense.dtype == np.float32 and np.isfinite(seg).all()
        if c.logits.startswith('byte'):
            n = int(c.logits[4])
            bits = seg.view(np.uint32) & np.uint32(0x7fffffff)
            assert len(np.unique(bits & ~np.uint32(0xFF << (8 * n)))) == 1 and len(np.unique(bits)) > 8, c.name
        if c.logits == 'denormal':
            assert (np.abs(seg) < 2.0 ** -126).all() and (seg != 0).all()
        if c.logits == 'negzero':
            assert (np.signbit(seg) & (seg == 0)).any()
        if c.logits in ('quant', 'equal'):
            assert len(np.unique(seg)) <= 40
    assert zero_present >= 3                                                 # a zero weight on a class that IS present
    assert {c.B for c in sc} == {1, 2, 3, 64, 65, 129} and {c.c2 for c in sc} == {2, 3, 5} and {c.proj for c in sc} == {True, False}
    assert {c.coord_weight for c in sc} == {10.0, 3.5} and {c.gout for c in sc} == {None, L.GOUT13}
    assert len(set(L.GOUT13)) == 12 and L.GOUT13.count(0.0) == 2
    assert {L.face_tables(c.table)[0].shape[0] for c in sc} >= {1, 255, 256, 257, 1538, L.F_MAX} and L.F_MAX == 3748
    assert {g for c in sc for g in c.geo} == {'same', 'knee', 'tiny', 'big', 'pzero', 'gzero', 'collinear', 'point'}
    assert 10 * sum(c.degenerate for c in sc) <= len(sc)                     # the 10 % cap
    for c in sc:
        for f in L.face_tables(c.table):
            assert f.dtype == np.int32 and f.min() >= 0 and f.max() < 778 and f.shape[0] <= L.F_MAX
            rep = (f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])
            assert rep.any() == (c.table == 'repeat') and (not rep.any() or c.degenerate)
    cnt = [np.bincount(f.reshape(-1), minlength=778) for f in L.face_tables('star300')]
    assert all(n[5] >= 300 for n in cnt)
    assert all((np.bincount(f.reshape(-1), minlength=778)[700:] == 0).all() for f in L.face_tables('novert'))


def test_restatement_agrees_with_the_oracle_in_float64():
    """the float64 values of the restatement against oracle/losses.py (float32 elementwise, float64 sums, pinned to G8 / G12) on the plain cases"""
    for c in L.dense_cases():
        if c.gout is not None or c.logits in ('big', 'byte3'):
            continue
        seg, dense, gt_seg, gt_dense = L.dense_inputs(c)
        ref = L.dense_reference(c)
        want = OL.dense_losses(seg, dense, gt_seg, gt_dense, c.class_weight, c.dense_weight)
        for k in ('seg', 'dense', 'lovasz'):
            assert abs(ref[k][0] - want[k]) <= 2e-6 * max(abs(want[k]), 1e-30), (c.name, k)
        g = OL.dense_loss_grads(seg, dense, gt_seg, gt_dense, c.class_weight, c.dense_weight)
        assert np.abs(ref['grad_seg'][0] - g['seg']).max() <= 1e-6 * np.abs(g['seg']).max(), c.name
        assert np.abs(ref['grad_dense'][0] - g['dense']).max() <= 2e-5 * np.abs(g['dense']).max(), c.name
    for c in L.stage_cases():
        if c.gout is not None or c.degenerate or c.B > 3:
            continue
        pred, gt, faces = L.stage_inputs(c)
        ref = L.stage_reference(c)
        want = OL.stage_losses(pred, gt, faces, c.coord_weight)
        for i, k in enumerate(OL.STAGE_KEYS):
            assert abs(ref['out13'][0][i] - want[k]) <= 2.0 * L.U * ref['out13'][1][i] + 1e-7 * abs(want[k]), (c.name, k)      # the oracle is a float32 evaluation: inside the bound S
        g = OL.stage_loss_grads(pred, gt, faces, c.coord_weight)
        for k, w in g.items():
            r, band = ref[k][0], ref[k][3]
            d = np.abs(r - w) if band is None else np.where(band, 0.0, np.abs(r - w))
            assert d.max() <= 2e-5 * np.abs(w).max(), (c.name, k)            # the oracle forms z in float32


def test_csr_is_the_wrappers():
    from dir_amd.models import loss as ML
    for kind in ('f1', 'f257', 'star300', 'repeat'):
        for f in L.face_tables(kind):
            off, idx = ML.vertex_face_csr(torch.from_numpy(f))
            a, b = L.csr(f)
            assert np.array_equal(off.numpy(), a) and np.array_equal(idx.numpy(), b)


def test_float32_references_stay_inside_a_quarter_of_c_and_ratios_are_reproduced(measured):
    """RATIOS is recorded 25 % above the measurement: every re-measured ratio lies in (ratio / 2, ratio] -- one that has grown fails here"""
    assert set(measured) == set(L.RATIOS) == set(L.CONSTANTS)
    for k, d in measured.items():
        for tag, r in d.items():
            assert L.RATIOS[k][tag] / 2.0 < r <= L.RATIOS[k][tag], (k, tag, r, L.RATIOS[k][tag])
        assert L.CONSTANTS[k] == 4.0 * max(L.RATIOS[k].values())
    stage = [k for k in L.RATIOS if k not in L.DENSE_KINDS]
    assert max(max(L.RATIOS[k].values()) for k in stage) < 1.5 * 1.25 / 1.05               # the stage's S is a running bound: a float32 evaluation cannot sit far outside it


def test_float32_references_pass_the_gate_inside_the_caps():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in L.stage_cases():
            ref = L.stage_reference(c)
            for got in (L.stage_eval(L.A32, c), L.torch_stage(c)):
                worst = L.stage_check(c, got, ref)
                assert max(worst.values()) <= 0.25 * 1.0001 or c.degenerate, (c.name, worst)
            if not c.degenerate:
                assert L.band_fraction(c, ref) <= 0.01, (c.name, L.band_fraction(c, ref))
        for c in L.dense_cases():
            assert max(L.dense_check(c, L.dense_eval(False, c)).values()) <= 0.25 * 1.0001, c.name
            assert max(L.dense_check(c, L.torch_dense(c), float64_scan=False).values()) <= 0.25 * 1.0001, c.name      # a float32 scan: every gate but grad_seg_scan
    finally:
        torch.set_num_threads(n)


def test_promised_zeros_of_a_collapsed_mesh():
    """every predicted vertex of one sample in one point: d = 0 and sgn(0) = 0 make every triangle contribution exactly 0 in the float32 evaluation -- the
    normal term is 0 and the mesh gradient is its SmoothL1 part, whatever grad_out says about the edge and normal slots"""
    case = next(c for c in L.stage_cases() if 'point' in c.geo)
    s = L.geo_sample(case, 'point')
    assert len({L.geo_sample(case, g) for g in case.geo}) == len(case.geo)
    got = L.stage_eval(L.A32, case)
    other = L.stage_eval(L.A32, case._replace(gout=tuple(0.0 if 8 <= k < 12 else v for k, v in enumerate(case.gout))))
    assert (got['scratch'][s, 10:12] == 0).all() and (got['scratch'][s, 8:10] > 0).all()
    for side in L.SIDES:
        k = 'pd_mesh_xyz_' + side
        assert np.isfinite(got[k]).all() and got[k][s].tobytes() == other[k][s].tobytes()
        assert np.abs(got[k][s]).max() > 0 or case.gout[6 + L.SIDES.index(side)] == 0      # (grad_out is 0 on the right hand's SmoothL1 slot)


@pytest.mark.parametrize('d', L.DEFECTS, ids=[d.name for d in L.DEFECTS])
def test_every_defect_is_rejected(d):
    """on EVERY case whose clean float32 result the defect changes in any bit the gate rejects it, but for the cases named, with the reason, in
    L.NOT_REJECTED"""
    moved, accepted, old_ok = L.defect_report(d)
    print('%s: changes %d cases, rejected on %d, accepted on %s; the old gates on this list %s it somewhere'
          % (d.name, len(moved), len(moved) - len(accepted), accepted, 'accept' if old_ok else 'reject'))
    assert len(L.DEFECTS) >= 12 and not L.EQUIVALENT and set(L.NOT_REJECTED) <= {x.name for x in L.DEFECTS}
    assert set(accepted) == set(L.NOT_REJECTED.get(d.name, {})) and len(moved) > len(accepted)
    assert old_ok == (d.name in L.OLD_GATES_ACCEPT)
