"""GPU parity of the fused layer3 bottleneck block (l3_chain.hip, dir_bottleneck_block_forward) against the two launches it replaces
(dir_amd/engine/backbone.py::BackboneOp._layers: blk['c2'], then BneckTailOp -- or, for the layer's last block, c3 with the residual;
models/backbone/resnet.py:126-140,122-124).  Those are themselves pinned against the oracle (test_gpu_conv_as.py, test_gpu_tail.py).  The
kernel accumulates in their K order and k-slot assignment and rounds y2 / out / y1n at their points, so every comparison is torch.equal.
Every fused call writes into buffers surrounded by sentinel values, which are checked afterwards: out and y1n are the only memory written."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from dir_amd import _capi, synth
from dir_amd import engine as E

pytestmark = pytest.mark.gpu
SEED = 4321
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PAD = 4096            # sentinel elements on either side of an output
SENTINEL = 3.25


def block_ops(seed, dt, fuse_next, big_shift=False):
    """(c2, c3, c1n | None) of one layer3 identity block with random parameters: channel-dependent weight magnitudes (a wrong k-slot or a swapped
    half changes the sum), negative BatchNorm scales included; big_shift: bn2's shift large and positive, so that bn2(conv2(0)) is far from zero"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)      # noqa: E731

    def conv(co, ci, k, shift0=0.0, **kw):
        mag = 0.25 + (torch.arange(ci, device='cuda') % 13).float() / 8.0
        w = rn(co, ci, k, k) * (2.0 / (ci * k * k)) ** 0.5 * mag[None, :, None, None]
        s = 0.5 + torch.rand(co, device='cuda', generator=g)
        s = torch.where(torch.rand(co, device='cuda', generator=g) < 0.3, -s, s)
        return E.ConvOp(w, dt, scale=s, shift=rn(co) * 0.3 + shift0, relu=True, **kw)
    c2 = conv(256, 256, 3, shift0=4.0 if big_shift else 0.0, pad=1)
    c3 = conv(1024, 256, 1)
    c1n = conv(256, 1024, 1) if fuse_next else None
    return c2, c3, c1n


def operands(seed, dt, B, H, offset=0.0):
    """y1 [B,H,16,256] with channel-dependent magnitudes and a value that differs from row to row and image to image; x [B,H,16,1024]"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    mag = 0.5 + (torch.arange(256, device='cuda') % 7).float() / 4.0
    rows = (torch.arange(B * H, device='cuda').float() * 0.37).reshape(B, H, 1, 1) % 3.0
    y1 = (torch.randn(B, H, 16, 256, device='cuda', generator=g) * mag + rows + offset).to(dt)
    x = torch.randn(B, H, 16, 1024, device='cuda', generator=g).to(dt)
    return y1, x


def reference(c2, c3, c1n, y1, x):
    """today's launches: the 3x3, then the tail (or conv3 with the residual)"""
    y2 = c2(y1)
    if c1n is not None:
        return E.BneckTailOp(c3, c1n)(y2, x)
    return c3(y2, residual=x), None


def guarded(shape, dt):
    flat = torch.full((2 * PAD + int(np.prod(shape)),), SENTINEL, device='cuda', dtype=dt)
    return flat, flat[PAD:-PAD].view(shape)


def fused(op, y1, x):
    """the fused launch through the C entry, into guarded buffers -> (out, y1n | None), sentinels checked"""
    B, H, W, _ = y1.shape
    fo, out = guarded((B, H, W, 1024), y1.dtype)
    fy, y1n = guarded((B, H, W, 256), y1.dtype) if op.c1n is not None else (None, None)
    assert op.supported(y1, x)
    _capi.check(_capi.lib().dir_bottleneck_block_forward(C.byref(op.params), _capi.ptr(y1), _capi.ptr(x), _capi.ptr(out), _capi.ptr(y1n), B, H, W,
                                                         _capi.stream_ptr()), 'dir_bottleneck_block_forward')
    torch.cuda.synchronize()
    for f in (fo, fy):
        if f is not None:
            edge = torch.cat([f[:PAD], f[-PAD:]]).float()
            assert float(edge.min()) == SENTINEL and float(edge.max()) == SENTINEL
    return out, y1n


def check(op, y1, x):
    ref_out, ref_y1n = reference(op.c2, op.c3, op.c1n, y1, x)
    out, y1n = fused(op, y1, x)
    assert torch.equal(out, ref_out)
    assert (y1n is None) == (ref_y1n is None)
    if y1n is not None:
        assert torch.equal(y1n, ref_y1n)
        assert float(ref_y1n.float().abs().max()) > 0.1
    assert float(ref_out.float().abs().max()) > 0.1
    return ref_out


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('fuse_next', [True, False])
@pytest.mark.parametrize('B', [1, 2, 5])
def test_fused_block_equals_two_launches(dt, fuse_next, B):
    """4, 8 and 20 tiles: fewer tiles than workgroups, the XCD-ordered walk (8) and the plain one, an odd count per XCD"""
    c2, c3, c1n = block_ops(SEED + B, dt, fuse_next)
    assert E.BneckBlockOp.applies(c2, c3, c1n, dt)
    op = E.BneckBlockOp(c2, c3, c1n)
    y1, x = operands(B * 10 + 1, dt, B, 16)
    check(op, y1, x)


@pytest.mark.parametrize('B,dt,fuse_next', [(65, torch.float16, True), (66, torch.bfloat16, True), (66, torch.float16, False)])
def test_more_tiles_than_workgroups(B, dt, fuse_next):
    """260 and 264 tiles on 256 CUs: some workgroups walk a second tile (the weight ring runs on into it, the patch takes T's place again), in
    the plain order (260) and in the XCD-aware one (264 = 8 x 33)"""
    assert torch.cuda.get_device_properties(0).multi_processor_count < 4 * B
    op = E.BneckBlockOp(*block_ops(SEED + B, dt, fuse_next))
    y1, x = operands(B, dt, B, 16)
    check(op, y1, x)


@pytest.mark.parametrize('fuse_next', [True, False])
def test_a_32_by_16_map(fuse_next):
    """H != 16: eight tiles of one image"""
    dt = torch.bfloat16
    op = E.BneckBlockOp(*block_ops(SEED + 11, dt, fuse_next))
    y1, x = operands(5, dt, 1, 32)
    check(op, y1, x)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_patch_outside_the_image_is_zero_not_a_clamped_row(dt):
    """conv2 pads y1 with zeros.  y1 is large and positive everywhere and bn2's shift is +4: a patch that held a clamped (repeated) row, or the
    neighbouring image's row, outside the image instead of zero would change every pixel of the top and bottom rows"""
    op = E.BneckBlockOp(*block_ops(SEED + 7, dt, True, big_shift=True))
    y1, x = operands(3, dt, 2, 16, offset=2.0)
    assert float(y1.float().mean()) > 1.0
    check(op, y1, x)
    y2_zero = op.c2(torch.zeros_like(y1))
    assert float(y2_zero.float().abs().mean()) > 0.5          # bn2(conv2(0)) != 0: a zero patch is not a zero y2


@pytest.mark.parametrize('fuse_next', [True, False])
def test_tile_and_image_borders(fuse_next):
    """rows 3 | 4, 7 | 8 and 11 | 12 of an image lie in different tiles, the last row of image b and the first of image b + 1 in neighbouring ones:
    every row gets its own constant on top of the noise, so a halo row taken from the wrong place (or the neighbouring image) shows"""
    dt = torch.float16
    op = E.BneckBlockOp(*block_ops(SEED + 13, dt, fuse_next))
    y1, x = operands(9, dt, 3, 16)
    r = y1.float().mean((2, 3))                               # [B, H]
    assert float((r[:, 3] - r[:, 4]).abs().min()) > 0.05 and float((r[:, 7] - r[:, 8]).abs().min()) > 0.05
    assert float((r[:, 11] - r[:, 12]).abs().min()) > 0.05 and float((r[:-1, 15] - r[1:, 0]).abs().min()) > 0.05
    check(op, y1, x)


def test_graph_replay_equals_eager():
    dt = torch.bfloat16
    op = E.BneckBlockOp(*block_ops(SEED + 1, dt, True))
    y1, x = operands(2, dt, 4, 16)
    eo, ey = (t.clone() for t in op(y1, x))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(y1, x)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        go, gy = op(y1, x)
    for _ in range(3):
        go.zero_(); gy.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(go, eo) and torch.equal(gy, ey)


def test_first_use_inside_a_graph_capture():
    """an engine that captures its first forward straight away makes the kernel's first launch INSIDE a stream capture (the stream is packed when
    the op is built, nothing is allocated or copied by the call).  Own process, so that no earlier test has launched the kernel."""
    code = r'''
import torch
from dir_amd import engine as E
g = torch.Generator(device='cuda').manual_seed(3)
dt = torch.bfloat16
rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
mk = lambda co, ci, k, **kw: E.ConvOp(rn(co, ci, k, k) * (2.0 / (ci * k * k)) ** 0.5, dt, scale=0.5 + torch.rand(co, device='cuda', generator=g), shift=rn(co) * 0.1, relu=True, **kw)
c2, c3, c1n = mk(256, 256, 3, pad=1), mk(1024, 256, 1), mk(256, 1024, 1)
op = E.BneckBlockOp(c2, c3, c1n)
y1, x = rn(2, 16, 16, 256).to(dt), rn(2, 16, 16, 1024).to(dt)
ro, ry = E.BneckTailOp(c3, c1n)(c2(y1), x)            # the two launches, eager
torch.cuda.synchronize()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        oo, oy = op(y1, x)                            # first launch of the fused kernel: inside the capture
    gr.replay()
torch.cuda.synchronize()
assert torch.equal(oo, ro) and torch.equal(oy, ry), 'captured first use differs'
print('OK')
'''
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_engine_falls_back_where_the_kernel_does_not_apply():
    dt = torch.bfloat16
    c2, c3, c1n = block_ops(SEED + 2, dt, True)
    op = E.BneckBlockOp(c2, c3, c1n)
    y1, x = operands(4, dt, 1, 16)
    assert op.supported(y1, x)
    assert not op.supported(y1[:, :6].contiguous(), x[:, :6].contiguous())                 # rows not a multiple of 4
    assert not op.supported(y1.float(), x.float())
    f2, f3, f1 = block_ops(SEED + 2, torch.float32, True)
    assert not E.BneckBlockOp.applies(f2, f3, f1, torch.float32)


@pytest.fixture(scope='module')
def dir_state():
    with open(os.path.join(GOLDEN, 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, SEED).items()}


def _forward_both(sd, dt, img):
    saved = E.BackboneOp.l3_chain
    res = []
    try:
        for on in (False, True):
            E.BackboneOp.l3_chain = on
            eng = E.DirEngine(sd, dtype=dt)
            blocks = eng.bb.layers[2]
            assert [('block' in b) for b in blocks] == [False] + [on] * 5
            if on:
                assert [b['block'].params.n_next for b in blocks[1:]] == [256, 256, 256, 256, 0]
            outs = eng.forward(img)
            res.append([{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs])
            torch.cuda.synchronize()
            del eng
    finally:
        E.BackboneOp.l3_chain = saved
    return res


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_whole_forward_is_bit_identical(dir_state, dt):
    img = torch.randn(3, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8))
    unfused, fused_ = _forward_both(dir_state, dt, img)
    n = 0
    for o0, o1 in zip(unfused, fused_):
        assert o0.keys() == o1.keys()
        for k, v in o0.items():
            assert torch.equal(v, o1[k]), k
            n += 1
    assert n > 20


def test_profile_records_keep_the_table_rows(dir_state):
    """the fused launch's record carries op = the 3x3 and covers = the launch it replaces: the layer list the tuning tables are keyed by is the
    same with the switch on and off"""
    saved = E.BackboneOp.l3_chain
    rows = []
    try:
        for on in (False, True):
            E.BackboneOp.l3_chain = on
            eng = E.DirEngine(dir_state, dtype=torch.bfloat16)
            img = torch.randn(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6))
            recs = eng._profiled_forwards(img, 1)
            ops = eng._layer_ops(recs)
            rows.append([[op.cout, op.cin, op.kh, op.kw, op.stride] for op in ops])
            if on:
                covered = [r for r in recs if r.get('covers') and r['op'] in [b['c2'] for b in eng.bb.layers[2]]]
                assert len(covered) == 5
            del eng
    finally:
        E.BackboneOp.l3_chain = saved
    assert rows[0] == rows[1] and len(rows[0]) == 52
