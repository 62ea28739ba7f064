"""GPU parity of the fused decoder Residual block (res_chain.hip, dir_residual_chain_forward) against the three launches it replaces
(dir_amd/engine/decoder.py::ResidualOp: conv1 with the pre-activation -> conv2 3x3 -> conv3 + skip_layer as one GEMM; models/backbone/hourglass.py:33-70).
The kernel accumulates in the same K order and k-slot assignment and rounds y1 / y2 / out at the same points, so every comparison here is
torch.equal: op level (both storage kinds, both map sizes, B = 1 / 3 / 64, output into a channel slice), the image border, the whole forward,
graph replay, the argument checks, and the row count of the shipped kernel table."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from dir_amd import _capi, synth
from dir_amd import engine as E

pytestmark = pytest.mark.gpu
SEED = 1234
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def residual_state(seed, cin=512, cout=256, big_shift=False):
    """random parameters of one hourglass.Residual under prefix 'r': negative BatchNorm scales included (a ReLU after a negative scale keeps what a
    positive one drops); big_shift: bn2's shift large and positive, so that conv1 + bn2 + ReLU of an all-zero pixel is far from zero"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)      # noqa: E731
    mid = cout // 2
    sd = {}
    for name, co, ci, k in (('skip_layer', cout, cin, 1), ('conv1', mid, cin, 1), ('conv2', mid, mid, 3), ('conv3', cout, mid, 1)):
        sd['r.%s.conv.weight' % name] = rn(co, ci, k, k) * (2.0 / (ci * k * k)) ** 0.5
        sd['r.%s.conv.bias' % name] = rn(co) * 0.2
    for name, c in (('bn1', cin), ('bn2', mid), ('bn3', mid)):
        w = 0.5 + torch.rand(c, device='cuda', generator=g)
        sd['r.%s.weight' % name] = torch.where(torch.rand(c, device='cuda', generator=g) < 0.3, -w, w)
        sd['r.%s.bias' % name] = rn(c) * 0.3 + (4.0 if big_shift and name == 'bn2' else 0.0)
        sd['r.%s.running_mean' % name] = rn(c) * 0.2
        sd['r.%s.running_var' % name] = 0.5 + torch.rand(c, device='cuda', generator=g)
    return sd


def both_paths(op, x, width, coff):
    """the block into channels [coff, coff + 256) of a `width`-channel buffer pre-filled with a pattern: (fused buffer, three-launch buffer)"""
    outs = []
    saved = E.ResidualOp.res_chain
    try:
        for fused in (True, False):
            E.ResidualOp.res_chain = fused
            buf = torch.full((x.shape[0], x.shape[1], x.shape[2], width), 3.25, device='cuda', dtype=x.dtype)
            if width == op.cout and coff == 0:
                buf = None
            y = op(x, out=buf, out_coff=coff)
            outs.append(y)
    finally:
        E.ResidualOp.res_chain = saved
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('hw', [32, 16])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_fused_block_equals_three_launches(dt, hw, B):
    op = E.ResidualOp(residual_state(SEED + hw + B), 'r', dt)
    assert op.chain is not None
    g = torch.Generator(device='cuda').manual_seed(B * 100 + hw)
    x = torch.randn(B, hw, hw, 512, device='cuda', generator=g).to(dt)
    for width, coff in ((512, 0), (512, 256), (256, 0)):
        fused, ref = both_paths(op, x, width, coff)
        assert fused.shape == ref.shape
        assert torch.equal(fused[..., coff:coff + 256], ref[..., coff:coff + 256]), (width, coff)
        if width > 256:       # the other channels of the buffer are bit-unchanged
            other = torch.cat([fused[..., :coff], fused[..., coff + 256:]], -1)
            assert torch.equal(other, torch.full_like(other, 3.25)), (width, coff)
    assert float(ref.float().abs().max()) > 0.1


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('hw', [32, 16])
def test_patch_outside_the_image_is_zero_not_conv1_of_zero(dt, hw):
    """conv2 pads y1 with zeros.  With bn2's shift at +4, relu(bn2(conv1(relu(bn1(anything))))) is O(1) everywhere: a patch that computed conv1 on
    clamped or zero pixels outside the image instead of holding zero would change every border pixel"""
    op = E.ResidualOp(residual_state(SEED + 7, big_shift=True), 'r', dt)
    x = torch.randn(2, hw, hw, 512, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)).to(dt)
    fused, ref = both_paths(op, x, 256, 0)
    assert torch.equal(fused, ref)
    # the border does depend on the padding: y1 of the zero-padded ring is not what conv1 would give there
    y1 = op.c1(x)
    assert float(y1.float().mean()) > 1.0


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_input_with_a_channel_stride(dt):
    """x as channels of a wider NHWC buffer is not what the engine passes today, but the C entry takes (in_cstride, in_coff): checked directly"""
    op = E.ResidualOp(residual_state(SEED + 9), 'r', dt)
    g = torch.Generator(device='cuda').manual_seed(11)
    wide = torch.randn(2, 16, 16, 640, device='cuda', generator=g).to(dt)
    x = wide[..., 64:576].contiguous()
    ref = both_paths(op, x, 256, 0)[1]
    out = torch.empty(2, 16, 16, 256, device='cuda', dtype=dt)
    _capi.check(_capi.lib().dir_residual_chain_forward(C.byref(op.chain), _capi.ptr(wide), _capi.ptr(out), 2, 16, 16, 640, 64, 256, 0, _capi.stream_ptr()),
                'dir_residual_chain_forward')
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_graph_replay_equals_eager():
    dt = torch.float16
    op = E.ResidualOp(residual_state(SEED + 1), 'r', dt)
    x = torch.randn(4, 32, 32, 512, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)).to(dt)
    eager = op(x).clone()
    out = torch.zeros(4, 32, 32, 512, device='cuda', dtype=dt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(x, out=out, out_coff=256)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        op(x, out=out, out_coff=256)
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[..., 256:], eager) and float(out[..., :256].float().abs().max()) == 0.0


def test_unsupported_shapes_are_refused_without_a_launch():
    L = _capi.lib()
    ok = (_capi.DT_F16, 512, 128, 256, 2, 32, 32, 512, 0, 256, 0)
    assert L.dir_residual_chain_supported(*ok) == 1
    bad = dict(dtype=(0, _capi.DT_F32), cin=(1, 1024), cin2=(1, 2304), mid=(2, 64), cout=(3, 512), odd_map=(5, 24), map8=(6, 8), cs=(7, 500), coff=(8, 4),
               ocs=(9, 128), ocoff=(10, 8))
    for name, (i, v) in bad.items():
        a = list(ok)
        a[i] = v
        if name == 'map8':
            a[5] = 8
        assert L.dir_residual_chain_supported(*a) == 0, name
    op = E.ResidualOp(residual_state(SEED), 'r', torch.float16)
    x = torch.zeros(1, 24, 24, 512, device='cuda', dtype=torch.float16)
    out = torch.full((1, 24, 24, 256), 2.0, device='cuda', dtype=torch.float16)
    L.dir_launch_log_reset()
    rc = L.dir_residual_chain_forward(C.byref(op.chain), _capi.ptr(x), _capi.ptr(out), 1, 24, 24, 512, 0, 256, 0, _capi.stream_ptr())
    assert rc == -1                                                    # DIR_E_INVALID
    buf = C.create_string_buffer(256)
    assert L.dir_launch_log_get(buf, 256) == 0                         # nothing was launched
    torch.cuda.synchronize()
    assert float(out.min()) == 2.0 and float(out.max()) == 2.0
    # the engine keeps the three launches for what the kernel does not take: an odd map size, fp32, another Cin
    y = op(x)
    assert y.shape == (1, 24, 24, 256)
    assert E.ResidualOp(residual_state(SEED), 'r', torch.float32).chain is None
    assert E.ResidualOp(residual_state(SEED, cin=1024), 'r', torch.float16).chain is None


@pytest.fixture(scope='module')
def dir_state():
    with open(os.path.join(GOLDEN, 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, SEED).items()}


def _forward_both(sd, dt, img):
    saved = E.ResidualOp.res_chain
    res = []
    try:
        for fused in (False, True):
            E.ResidualOp.res_chain = fused
            eng = E.DirEngine(sd, dtype=dt)
            assert (eng.res['enhance_layer3'].chain is not None) == fused and eng.res['skip_layer4'].chain is None
            outs = eng.forward(img)
            res.append([{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs])
            torch.cuda.synchronize()
            del eng
    finally:
        E.ResidualOp.res_chain = saved
    return res


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B', [64, 3])
def test_whole_forward_is_bit_identical(dir_state, dt, B):
    img = torch.randn(B, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8))
    unfused, fused = _forward_both(dir_state, dt, img)
    n = 0
    for o0, o1 in zip(unfused, fused):
        assert o0.keys() == o1.keys()
        for k, v in o0.items():
            assert torch.equal(v, o1[k]), k
            n += 1
    assert n > 20


def test_engine_op_list_matches_the_shipped_table(dir_state):
    """four blocks fused: 60 conv-family ops become 52, and dir_amd/tuning/gfx950_bf16_b64_throughput.json must have been re-made with them"""
    with open(os.path.join(ROOT, 'dir_amd', 'tuning', 'gfx950_bf16_b64_throughput.json')) as f:
        shipped = json.load(f)
    eng = E.DirEngine(dir_state, dtype=torch.bfloat16)
    img = torch.randn(64, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6))
    eng.import_tuning(img, shipped['table'])                            # raises ValueError when rows and ops differ
    table = eng.export_tuning(64)
    assert len(table) == len(shipped['table']) == 52
    assert sum(1 for r in table if r[:5] == [256, 512, 3, 3, 1]) == 4
