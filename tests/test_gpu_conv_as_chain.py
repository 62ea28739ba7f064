"""GPU parity of the chained mode of the activation-stationary kernel (conv_as.hip, dir_conv2d_as_chain_forward): a 3x3 256-channel layer on the
32-wide map and the 1x1 that alone reads it as ONE launch -- models/dir.py:474-476 (conv_final.0 -> conv_final.3) and models/dir.py:425-433 (the
merged seg | dense 3x3 -> their 1x1s, fp32 out).  Through the C ABI: BIT FOR BIT against the two launches it replaces (dir_conv2d_as_forward (2, 4),
then dir_conv2d_forward), sentinel channels around the output slice included, and against the fp64 oracle evaluated with the intermediate map
rounded to the storage kind (tolerances of test_gpu_conv_as.py).  Shapes: the smallest that can still go wrong -- one tile whose halo rows both
lie outside the image; two tiles per image (a halo row from the neighbouring tile, never from the neighbouring image) with 6 tiles (linear tile
map) and 8 (XCD map); one input slab and four."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import relerr
from dir_amd import _capi, synth
from dir_amd import engine as E
from oracle import nnops as N

pytestmark = pytest.mark.gpu
SEED = 1234
W, CMID = 32, 256
GEOMS = [(1, 4), (3, 8), (4, 8)]      # (B, H): 1 tile | 6 tiles, linear map | 8 tiles, XCD map


def _round(a, tdt):
    return torch.from_numpy(np.asarray(a, np.float32)).to(tdt).float().numpy()


@functools.lru_cache(maxsize=None)
def _params(Cin, dt, big=False):
    """host parameters of one pair (rounded to the storage kind where the kernels read them so); negative stage-1 scales included"""
    tag = 'aschain.%d' % Cin
    w3 = _round(synth.synth_input(tag + '.w3', (CMID, Cin, 3, 3), SEED) * np.float32(np.sqrt(2.0 / (9 * Cin))), dt)
    s1 = synth.synth_input(tag + '.s1', (CMID,), SEED, kind='uniform', lo=0.5, hi=1.5)
    s1 = np.where(np.arange(CMID) % 5 == 3, -s1, s1).astype(np.float32) * np.float32(3e5 if big else 1.0)
    b1 = synth.synth_input(tag + '.b1', (CMID,), SEED) * np.float32(0.3)
    wa = _round(synth.synth_input(tag + '.wa', (256, CMID, 1, 1), SEED) * np.float32(np.sqrt(2.0 / CMID)), dt)
    sa = synth.synth_input(tag + '.sa', (256,), SEED, kind='uniform', lo=0.5, hi=1.5)
    ba = synth.synth_input(tag + '.ba', (256,), SEED) * np.float32(0.3)
    wb = _round(synth.synth_input(tag + '.wb', (6, CMID, 1, 1), SEED) * np.float32(np.sqrt(2.0 / CMID)), dt)
    bb = synth.synth_input(tag + '.bb', (6,), SEED) * np.float32(0.3)
    return dict(w3=w3, s1=s1, b1=b1, wa=wa, sa=sa, ba=ba, wb=wb, bb=bb)


@functools.lru_cache(maxsize=None)
def _input(B, H, Cin, dt):
    return _round(synth.synth_input('aschain.x.%d_%d_%d' % (B, H, Cin), (B, Cin, H, W), SEED), dt)


@functools.lru_cache(maxsize=None)
def _oracle_mid(B, H, Cin, dt):
    """fp64: scale1 * conv3x3(x) + shift1 (before the activation and the rounding), computed once per geometry"""
    p = _params(Cin, dt)
    y = N.conv2d(_input(B, H, Cin, dt).astype(np.float64), p['w3'].astype(np.float64), None, 1, 1)
    return y * p['s1'].astype(np.float64).reshape(1, -1, 1, 1) + p['b1'].astype(np.float64).reshape(1, -1, 1, 1)


def _oracle(B, H, Cin, dt, relu1, w2, s2, b2):
    t = _oracle_mid(B, H, Cin, dt)
    if relu1:
        t = np.maximum(t, 0)
    t = _round(t, dt).astype(np.float64)                       # the intermediate map as the kernels hold it
    y = N.conv2d(t, w2.astype(np.float64), None, 1, 0)
    if s2 is not None:
        y = y * s2.astype(np.float64).reshape(1, -1, 1, 1)
    return y + b2.astype(np.float64).reshape(1, -1, 1, 1)


def _dev(a, tdt=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().to(tdt).contiguous()


class Pair(object):
    """device operands of one pair, for both paths"""
    def __init__(self, Cin, dt, relu1, w2, s2, b2, f32_out, big=False):
        p = _params(Cin, dt, big)
        self.Cin, self.dt, self.relu1, self.f32_out, self.cout2 = Cin, dt, relu1, f32_out, w2.shape[0]
        self.w3 = _dev(p['w3'].transpose(0, 2, 3, 1), dt)       # [Cout][kh][kw][Cin]
        self.w2 = _dev(w2.transpose(0, 2, 3, 1), dt)
        self.s1, self.b1, self.s2, self.b2 = _dev(p['s1']), _dev(p['b1']), _dev(s2), _dev(b2)
        self.w3_as = E.pack_as_weights(self.w3, 2)
        if f32_out:
            wp = torch.zeros(128, 1, 1, CMID, device='cuda', dtype=dt)
            wp[:self.cout2] = self.w2
            self.w2_as = E.pack_as_weights(wp, 1)
        else:
            self.w2_as = E.pack_as_weights(self.w2, 2)

    def desc3(self, B, H):
        return _capi.ConvDesc(B, H, W, self.Cin, self.Cin, 0, CMID, CMID, 0, 0, 0, 3, 3, 1, 1, E._dt(self.dt), E._dt(self.dt),
                              _capi.CONV_RELU if self.relu1 else 0, 0, 0, 1.0)

    def new_out(self, B, H):
        """(buffer, channel stride, channel offset): 16-bit into channels [64, 320) of a 384-channel buffer of sentinels; fp32 [B,H,W,cout2]"""
        if self.f32_out:
            return torch.full((B, H, W, self.cout2), 3.0, device='cuda', dtype=torch.float32), self.cout2, 0
        return torch.full((B, H, W, self.cout2 + 128), 3.0, device='cuda', dtype=self.dt), self.cout2 + 128, 64

    def chained(self, x):
        B, H = x.shape[:2]
        L = _capi.lib()
        out, cs, co = self.new_out(B, H)
        odt = _capi.DT_F32 if self.f32_out else E._dt(self.dt)
        assert L.dir_conv2d_as_chain_supported(self.desc3(B, H), self.cout2, odt) == 1
        L.dir_launch_log_reset()
        _capi.check(L.dir_conv2d_as_chain_forward(self.desc3(B, H), _capi.ptr(x), _capi.ptr(self.w3_as), _capi.ptr(self.s1), _capi.ptr(self.b1),
                                                  _capi.ptr(self.w2_as), _capi.ptr(self.s2), _capi.ptr(self.b2), self.cout2, 0,
                                                  _capi.ptr(out), cs, co, odt, _capi.stream_ptr()), 'dir_conv2d_as_chain_forward')
        buf = C.create_string_buffer(256)
        assert L.dir_launch_log_get(buf, 256) == 1 and 'conv_as_kernel' in buf.value.decode()      # one launch
        torch.cuda.synchronize()
        return out

    def two_launches(self, x):
        B, H = x.shape[:2]
        L = _capi.lib()
        mid = torch.empty(B, H, W, CMID, device='cuda', dtype=self.dt)
        _capi.check(L.dir_conv2d_as_forward(self.desc3(B, H), _capi.ptr(x), _capi.ptr(self.w3_as), _capi.ptr(self.s1), _capi.ptr(self.b1), None,
                                            _capi.ptr(mid), 2, 4, _capi.stream_ptr()), 'dir_conv2d_as_forward')
        out, cs, co = self.new_out(B, H)
        d = _capi.ConvDesc(B, H, W, CMID, CMID, 0, self.cout2, cs, co, 0, 0, 1, 1, 1, 0, E._dt(self.dt),
                           _capi.DT_F32 if self.f32_out else E._dt(self.dt), 0, 0, 0, 1.0)
        _capi.check(L.dir_conv2d_forward(d, _capi.ptr(mid), _capi.ptr(self.w2), _capi.ptr(self.s2), _capi.ptr(self.b2), None, None, None,
                                         _capi.ptr(out), _capi.stream_ptr()), 'dir_conv2d_forward')
        torch.cuda.synchronize()
        return out, mid


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('Cin', [64, 256])
@pytest.mark.parametrize('geom', GEOMS)
def test_chain_equals_the_two_launches_bit_for_bit_and_matches_the_oracle(geom, Cin, dt):
    B, H = geom
    p = _params(Cin, dt)
    x = _dev(_input(B, H, Cin, dt).transpose(0, 2, 3, 1), dt)
    tol = 1e-2 if dt == torch.bfloat16 else 2e-3
    for relu1 in (True, False):
        # (second layer, scale2, shift2, fp32 out): 256 channels into a slice with and without scale2, and the 6-channel fp32 head (no scale2)
        for w2, s2, b2, f32_out in ((p['wa'], p['sa'], p['ba'], False), (p['wa'], None, p['ba'], False), (p['wb'], None, p['bb'], True)):
            if s2 is None and not f32_out and relu1:
                continue
            pair = Pair(Cin, dt, relu1, w2, s2, b2, f32_out)
            got = pair.chained(x)
            want, _ = pair.two_launches(x)
            assert torch.equal(got, want), (geom, Cin, dt, relu1, f32_out, s2 is None)      # incl. the sentinel channels around the slice
            if not f32_out:
                assert bool((got[..., :64] == 3.0).all()) and bool((got[..., 64 + 256:] == 3.0).all())
                got = got[..., 64:64 + 256]
            ref = _oracle(B, H, Cin, dt, relu1, w2, s2, b2)
            err = relerr(got.float().cpu().numpy().transpose(0, 3, 1, 2), ref)
            print('B=%d H=%d Cin=%d %s relu1=%d N2=%d scale2=%d relerr %.3e' % (B, H, Cin, dt, relu1, w2.shape[0], s2 is not None, err))
            assert err < tol


def test_f16_intermediate_saturates_at_65504_as_the_separate_launch_stores_it():
    """stage-1 scales of +-3e5 x [0.5, 1.5) drive the 3x3's map far past the f16 range: the separate launch stores +-65504 (MODE.FP16_OVFL), and
    the chained kernel must round its in-register intermediate the same way, with and without the ReLU"""
    B, H, Cin, dt = 3, 8, 64, torch.float16
    p = _params(Cin, dt, big=True)
    x = _dev(_input(B, H, Cin, dt).transpose(0, 2, 3, 1), dt)
    for relu1 in (True, False):
        for w2, s2, b2, f32_out in ((p['wa'], p['sa'], p['ba'], False), (p['wb'], None, p['bb'], True)):
            pair = Pair(Cin, dt, relu1, w2, s2, b2, f32_out, big=True)
            want, mid = pair.two_launches(x)
            assert bool(torch.isfinite(mid).all()) and float(mid.max()) == 65504.0 and (relu1 or float(mid.min()) == -65504.0)
            assert int((mid.abs() == 65504.0).sum()) > mid.numel() // 4      # the case really is about saturated values
            assert torch.equal(pair.chained(x), want), (relu1, f32_out)


def test_refusals_come_before_any_launch():
    L = _capi.lib()
    bf, f32 = _capi.DT_BF16, _capi.DT_F32

    def desc(B=2, H=8, Wd=32, Cin=64, Cmid=256, stride=1, dt=bf):
        return _capi.ConvDesc(B, H, Wd, Cin, Cin, 0, Cmid, Cmid, 0, 0, 0, 3, 3, stride, 1, dt, dt, 0, 0, 0, 1.0)
    assert L.dir_conv2d_as_chain_supported(desc(), 256, bf) == 1 and L.dir_conv2d_as_chain_supported(desc(), 6, f32) == 1
    one = C.c_void_p(16)
    bad = {'W = 24': desc(H=16, Wd=24), 'Cmid = 128': desc(Cmid=128), 'stride 2': desc(stride=2), 'fp32 storage': desc(dt=f32),
           'H W not a multiple of 128': desc(H=2), 'Cin not a multiple of 64': desc(Cin=96)}
    for name, d in bad.items():
        for cout2, odt in ((256, d.in_dtype), (6, f32)):
            assert L.dir_conv2d_as_chain_supported(d, cout2, odt) == 0, name
            L.dir_launch_log_reset()
            rc = L.dir_conv2d_as_chain_forward(d, one, one, None, None, one, None, None, cout2, 0, one, 0, 0, odt, None)
            assert rc != 0 and b'not supported' in L.dir_last_error(), name
            assert L.dir_launch_log_get(C.create_string_buffer(64), 64) == 0, name
    # the second layer: 256 channels in the storage kind, or 2 / 4 / 6 / 8 as fp32; output slices aligned to the stores
    for cout2, odt in ((128, bf), (256, _capi.DT_F16), (256, f32), (5, f32), (10, f32), (0, f32)):
        assert L.dir_conv2d_as_chain_supported(desc(), cout2, odt) == 0, (cout2, odt)
    L.dir_launch_log_reset()
    assert L.dir_conv2d_as_chain_forward(desc(), one, one, None, None, one, None, None, 256, 0, one, 260, 0, bf, None) != 0 and b'output slice' in L.dir_last_error()
    assert L.dir_conv2d_as_chain_forward(desc(), one, one, None, None, one, None, None, 6, 0, one, 8, 3, f32, None) != 0 and b'output slice' in L.dir_last_error()
    assert L.dir_conv2d_as_chain_forward(desc(), one, one, None, None, None, None, None, 6, 0, one, 0, 0, f32, None) != 0 and b'null pointer' in L.dir_last_error()
    assert L.dir_launch_log_get(C.create_string_buffer(64), 64) == 0


def test_first_use_inside_a_graph_capture():
    """The chained instantiations opt into > 64 KB of dynamic LDS (hipFuncSetAttribute) on their first launch, and an engine that captures its
    first forward straight away makes that launch INSIDE a stream capture.  Own process, so that no earlier test has launched them."""
    import os
    import subprocess
    import sys
    code = r'''
import torch
from dir_amd import engine as E
g = torch.Generator(device='cuda').manual_seed(3)
dt = torch.bfloat16
rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
c3 = E.ConvOp(rn(256, 64, 3, 3) * 0.05, dt, pad=1, scale=torch.ones(256, device='cuda'), shift=rn(256) * 0.1, relu=True)
ca = E.ConvOp(rn(256, 256, 1, 1) * 0.05, dt, shift=rn(256) * 0.1)
cb = E.ConvOp(rn(6, 256, 1, 1) * 0.05, dt, shift=rn(6) * 0.1, out_dtype=torch.float32)
pa, pb = E.ConvChainOp(c3, ca), E.ConvChainOp(c3, cb)
assert pa.w is not None and pb.w is not None
x = rn(2, 8, 32, 64).to(dt)
E.ConvChainOp.head_chain = False
ra, rb = pa(x).clone(), pb(x).clone()                 # the two launches each, eager
E.ConvChainOp.head_chain = True
torch.cuda.synchronize()
oa, ob = torch.empty_like(ra), torch.empty_like(rb)
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        pa(x, out=oa); pb(x, out=ob)                  # first launch of both chained instantiations: inside the capture
    gr.replay()
torch.cuda.synchronize()
assert torch.equal(oa, ra) and torch.equal(ob, rb), 'captured first use differs'
print('OK')
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
