"""GPU: the loss kernels of csrc/loss.hip per element -- dir_stage_losses_forward (13 batch scalars and the per-sample table scratch[B][13]),
dir_stage_losses_backward (every element of the nine gradient tensors), dir_dense_losses_forward (3 scalars) and dir_dense_losses_backward
(every element of grad_seg and grad_dense) -- at the cases of tests/helpers/loss_cases.py: float64 references, error scales S and constants c
measured on float32 CPU references, never on the kernels (described and pinned there and in tests/test_loss_cases_ref.py).

Every case goes through the C ABI with its workspace and scratch pre-filled with 0xFF bytes, its outputs between guard floats that must keep
their bits, and runs twice to the same bits.

Measured on the MI355X (information, not a bound; worst |got - ref64| over a list in units of the tolerance, i.e. of c 2^-24 S + floor): stage
forward scratch 0.073 (SmoothL1), 0.14 (edge), 0.20 (normal), out13 0.092 / 0.18 / 0.20; stage backward joint_uv 0.18, mesh_uv 0.14, joint_xyz
0.20, mesh_xyz 0.20, offset 0.20; dense seg 0.023, dense 0.026, lovasz 0.024, grad_seg 0.12, grad_seg_scan (the float64-scan gate that tells a
reversed tie) 0.18, grad_dense 0.16 -- the float32 CPU references sit at 0.2 by construction (constants recorded 25 % above the measurement), so the
kernels are as close to float64 as a float32 evaluation gets.  Denormal errors keep their order (no flush), 3748 faces (150 KB of LDS) ran and 3749
raised.  No kernel defect was found."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from dir_amd import _capi
from dir_amd.models import loss as ML

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import loss_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu
FILL, GUARD = -7.75e33, 64


def _dev(a, device='cuda'):
    return torch.from_numpy(np.array(a)).to(device)                      # a copy: the helper's inputs are read-only


class Guarded(object):
    """n floats between two rows of GUARD floats holding FILL"""

    def __init__(self, n, device='cuda'):
        self.n, self.buf = n, torch.full((n + 2 * GUARD,), FILL, device=device, dtype=torch.float32)
        self.out = self.buf[GUARD:GUARD + n]

    def take(self, shape):
        fill = torch.tensor(FILL, dtype=torch.float32)
        assert bool((self.buf[:GUARD].cpu() == fill).all()) and bool((self.buf[GUARD + self.n:].cpu() == fill).all()), 'guard floats written'
        return self.out.cpu().numpy().reshape(shape).copy()


def _bytes_ff(n, device='cuda'):
    return torch.full((n,), 255, device=device, dtype=torch.uint8)


def _pair(ts):
    return (C.c_void_p * 2)(*[None if t is None else t.data_ptr() for t in ts])


def run_stage(case, device='cuda', faces=None, forward=True, backward=True):
    """forward and backward of one stage case -> {name: numpy}"""
    pred, gt, tables = L.stage_inputs(case)
    tables = tables if faces is None else faces
    B = case.B
    keep = {k: _dev(v, device) for d in (pred, gt) for k, v in d.items()}
    fs = [_dev(f, device) for f in tables]
    g = _capi.LossTarget()
    for field, prefix in (('joint_2d', 'joint_2d_'), ('mesh_2d', 'mesh_2d_'), ('joint_3d', 'joint_3d_'), ('mesh_3d', 'mesh_3d_'), ('center', 'center_')):
        setattr(g, field, _pair([keep[prefix + s] for s in L.SIDES]))
    g.faces, g.c2, g.n_faces = _pair(fs), case.c2, int(tables[0].shape[0])

    def lp(forward):
        p = _capi.LossPred()
        for field, prefix in (('joint_uv', 'pd_joint_uv_'), ('joint_xyz', 'pd_joint_xyz_'), ('mesh_xyz', 'pd_mesh_xyz_')):
            setattr(p, field, _pair([keep[prefix + s] for s in L.SIDES]))
        if forward and case.proj:
            p.mesh_uv, p.proj = _pair([None, None]), _pair([keep['pd_proj_' + s] for s in L.SIDES])
        else:
            p.mesh_uv, p.proj = _pair([keep['pd_mesh_uv_' + s] for s in L.SIDES]), _pair([None, None])
        p.offset = keep['pd_offset'].data_ptr()
        return p
    befores = {k: v.clone() for k, v in keep.items()}
    out = {}
    with torch.cuda.device(device):
        if forward:
            raw = _bytes_ff(8 * (B * 13 + 2 * GUARD), device)
            scratch = raw.view(torch.float64)[GUARD:GUARD + B * 13]
            o13 = Guarded(13, device)
            p = lp(True)
            _capi.check(_capi.lib().dir_stage_losses_forward(C.byref(p), C.byref(g), float(case.coord_weight), _capi.ptr(scratch), _capi.ptr(o13.out), B,
                                                             _capi.stream_ptr()), 'dir_stage_losses_forward')
            torch.cuda.synchronize()
            assert bool((raw[:8 * GUARD] == 255).all()) and bool((raw[8 * (GUARD + B * 13):] == 255).all()), 'scratch guard written'
            out['scratch'], out['out13'] = scratch.cpu().numpy().reshape(B, 13).copy(), o13.take((13,))
        if backward:
            p, o = lp(False), _capi.LossPredGrad()
            gs = {k: Guarded(pred[k].size, device) for k in L.STAGE_GRADS}
            for field, prefix in (('joint_uv', 'pd_joint_uv_'), ('mesh_uv', 'pd_mesh_uv_'), ('joint_xyz', 'pd_joint_xyz_'), ('mesh_xyz', 'pd_mesh_xyz_')):
                setattr(o, field, _pair([gs[prefix + s].out for s in L.SIDES]))
            o.offset = gs['pd_offset'].out.data_ptr()
            csr = [[_dev(a, device) for a in L.csr(f)] for f in tables]
            offs, idxs = _pair([c[0] for c in csr]), _pair([c[1] for c in csr])
            go = None if case.gout is None else _dev(np.asarray(case.gout, np.float32), device)
            _capi.check(_capi.lib().dir_stage_losses_backward(C.byref(p), C.byref(g), float(case.coord_weight), _capi.ptr(go), C.byref(offs), C.byref(idxs),
                                                              C.byref(o), B, _capi.stream_ptr()), 'dir_stage_losses_backward')
            torch.cuda.synchronize()
            for k in L.STAGE_GRADS:
                out[k] = gs[k].take(pred[k].shape)
    assert all(torch.equal(v, befores[k]) for k, v in keep.items()), 'an input was written'
    return out


def run_dense(case):
    seg, dense, gt_seg, gt_dense = (_dev(a) for a in L.dense_inputs(case))
    B, S, H, W = case.B, case.S, case.H, case.W
    lib = _capi.lib()
    cw = (C.c_float * 3)(*case.class_weight)
    go = None if case.gout is None else _dev(np.asarray(case.gout, np.float32))
    nf, nb = lib.dir_dense_losses_workspace_bytes(B, S), lib.dir_dense_losses_backward_workspace_bytes(B, S)
    assert nf > 0 and nb > 0
    wf, wb = _bytes_ff(nf + 512), _bytes_ff(nb + 512)
    o3, gseg, gdense = Guarded(3), Guarded(seg.numel()), Guarded(dense.numel())
    _capi.check(lib.dir_dense_losses_forward(_capi.ptr(seg), _capi.ptr(dense), _capi.ptr(gt_seg), _capi.ptr(gt_dense), cw, float(case.dense_weight),
                                             C.c_void_p(wf.data_ptr() + 256), nf, _capi.ptr(o3.out), B, S, H, W, _capi.stream_ptr()), 'dir_dense_losses_forward')
    _capi.check(lib.dir_dense_losses_backward(_capi.ptr(seg), _capi.ptr(dense), _capi.ptr(gt_seg), _capi.ptr(gt_dense), cw, float(case.dense_weight), _capi.ptr(go),
                                              C.c_void_p(wb.data_ptr() + 256), nb, _capi.ptr(gseg.out), _capi.ptr(gdense.out), B, S, H, W, _capi.stream_ptr()),
                'dir_dense_losses_backward')
    torch.cuda.synchronize()
    for w, n in ((wf, nf), (wb, nb)):
        assert bool((w[:256] == 255).all()) and bool((w[256 + n:] == 255).all()), 'workspace overrun'
    o = o3.take((3,))
    return {'seg': o[0], 'dense': o[1], 'lovasz': o[2], 'grad_seg': gseg.take(seg.shape), 'grad_dense': gdense.take(dense.shape)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('case', L.stage_cases(), ids=[c.name for c in L.stage_cases()])
def test_stage_per_element(case):
    got = run_stage(case)
    again = run_stage(case)
    assert all(_same_bits(got[k], again[k]) for k in got), case.name
    worst = L.stage_check(case, got, what='MI355X')
    print('%s worst ratio / c: %s' % (case.name, {k: '%.3g' % v for k, v in sorted(worst.items())}))


@pytest.mark.parametrize('case', L.dense_cases(), ids=[c.name for c in L.dense_cases()])
def test_dense_per_element(case):
    got = run_dense(case)
    again = run_dense(case)
    assert all(_same_bits(got[k], again[k]) for k in got), case.name
    worst = L.dense_check(case, got, what='MI355X')
    print('%s worst ratio / c: %s' % (case.name, {k: '%.3g' % v for k, v in sorted(worst.items())}))


def test_promised_zeros_of_a_collapsed_mesh():
    """degenerate class: one sample's predicted mesh in one point -- normal term exactly 0, and a mesh gradient that is its SmoothL1 part bit for bit,
    i.e. the bits of the same call with the edge and normal grad_out slots at 0"""
    case = next(c for c in L.stage_cases() if 'point' in c.geo)
    s = L.geo_sample(case, 'point')
    got = run_stage(case)
    other = run_stage(case._replace(gout=tuple(0.0 if 8 <= k < 12 else v for k, v in enumerate(case.gout))))
    assert (got['scratch'][s, 10:12] == 0).all() and (got['scratch'][s, 8:10] > 0).all()
    for side in L.SIDES:
        k = 'pd_mesh_xyz_' + side
        assert _same_bits(got[k][s], other[k][s])
        assert np.abs(got[k][s]).max() > 0 or case.gout[6 + L.SIDES.index(side)] == 0      # (grad_out is 0 on the right hand's SmoothL1 slot)


def test_wrapper_returns_the_abi_bits():
    """dir_amd.models.loss (its own scratch, workspace and CSR lists) gives the bits of the direct calls, forward with projection included"""
    for name in ('b2_c3', 'b3_c3_proj'):
        case = next(c for c in L.stage_cases() if c.name == name)
        pred, gt, faces = L.stage_inputs(case)
        got = run_stage(case)
        cu = lambda d: {k: _dev(v) for k, v in d.items()}  # noqa: E731
        target, meta = cu({k: v for k, v in gt.items() if not k.startswith('center')}), cu({k: v for k, v in gt.items() if k.startswith('center')})
        ft = [torch.from_numpy(f) for f in faces]
        go = None if case.gout is None else _dev(np.asarray(case.gout, np.float32))
        fwd = {k: v for k, v in pred.items() if not (case.proj and 'mesh_uv' in k)}
        assert _same_bits(ML.stage_losses(cu(fwd), target, meta, ft, case.coord_weight).cpu().numpy(), got['out13'])
        grads = ML.stage_loss_grads(cu(pred), target, meta, ft, case.coord_weight, grad_out=go)
        assert all(_same_bits(grads[k].cpu().numpy(), got[k]) for k in L.STAGE_GRADS)
    case = next(c for c in L.dense_cases() if c.gout is not None and c.B * c.S * c.S > 8192)
    got = run_dense(case)
    t = [_dev(a) for a in L.dense_inputs(case)]
    o = ML.dense_losses(*t, class_weight=case.class_weight, dense_weight=case.dense_weight).cpu().numpy()
    assert _same_bits(o, np.array([got['seg'], got['dense'], got['lovasz']], np.float32))
    gs, gd = ML.dense_loss_grads(*t, class_weight=case.class_weight, dense_weight=case.dense_weight, grad_out=_dev(np.asarray(case.gout, np.float32)))
    assert _same_bits(gs.cpu().numpy(), got['grad_seg']) and _same_bits(gd.cpu().numpy(), got['grad_dense'])


def test_one_face_more_than_lds_admits_is_an_error():
    """F_MAX faces run (the fmax case above); with F_MAX + 1 dir_stage_losses_backward must raise DirHipError and launch nothing"""
    case = next(c for c in L.stage_cases() if c.name == 'fmax')
    faces = tuple(np.ascontiguousarray(np.concatenate([f, f[:1]])) for f in L.face_tables(case.table))
    assert faces[0].shape[0] == L.F_MAX + 1
    _capi.lib().dir_launch_log_reset()
    with pytest.raises(_capi.DirHipError):
        run_stage(case, faces=faces, forward=False)
    buf = C.create_string_buffer(1024)
    _capi.lib().dir_launch_log_get(buf, 1024)
    assert buf.value == b''


def test_stage_backward_on_a_second_device_after_the_first():
    """the dynamic-LDS limit of stage_loss_bwd_kernel is raised per device: device 1 after device 0 in one process, 74 KB of LDS at 1538 faces"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    case = next(c for c in L.stage_cases() if c.name == 'b2_c3')
    first = run_stage(case, 'cuda:0')
    second = run_stage(case, 'cuda:1')
    L.stage_check(case, second, what='device 1')
    assert all(_same_bits(first[k], second[k]) for k in first)
    assert all(_same_bits(first[k], v) for k, v in run_stage(case, 'cuda:0').items())
