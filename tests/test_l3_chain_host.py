"""CPU-only: the host side of the fused layer3 bottleneck block (l3_chain.hip, dir_bottleneck_block_forward).  Geometry the kernel does not
take is refused with the library's error code before anything touches a device, and the weight stream dir_amd/packing.py::pack_l3_stream
builds is the layout include/dir_hip.h documents, element by element."""
import ctypes as C

import torch

from dir_amd import _capi, packing


def test_unsupported_geometry_is_refused_before_any_launch():
    L = _capi.lib()
    bf, f16, f32 = _capi.DT_BF16, _capi.DT_F16, _capi.DT_F32
    ok = dict(dtype=bf, planes=256, n_next=256, B=2, H=16, W=16)
    sup = lambda **kw: L.dir_bottleneck_block_supported(*[dict(ok, **kw)[k] for k in ('dtype', 'planes', 'n_next', 'B', 'H', 'W')])      # noqa: E731
    assert sup() == 1 and sup(dtype=f16) == 1 and sup(n_next=0) == 1 and sup(H=32) == 1 and sup(H=4, B=1) == 1
    bad = {'fp32': dict(dtype=f32), 'planes 128': dict(planes=128), 'n_next 128': dict(n_next=128), 'n_next 512': dict(n_next=512),
           'W 32': dict(W=32), 'W 8': dict(W=8), 'rows not a multiple of 4': dict(H=6), 'H 0': dict(H=0), 'B 0': dict(B=0)}
    one = C.c_void_p(16)

    def params(planes=256, n_next=256, dtype=bf, wstream=16, scale1n=16):
        return _capi.BneckBlockParams(wstream, 16, 16, 16, 16, scale1n, 16, planes, n_next, dtype)
    for name, kw in bad.items():
        assert sup(**kw) == 0, name
        a = dict(ok, **kw)
        L.dir_launch_log_reset()
        rc = L.dir_bottleneck_block_forward(C.byref(params(a['planes'], a['n_next'], a['dtype'])), one, one, one, one, a['B'], a['H'], a['W'], None)
        assert rc == -1 and b'unsupported' in L.dir_last_error(), name                      # DIR_E_INVALID
        assert L.dir_launch_log_get(C.create_string_buffer(64), 64) == 0, name
    L.dir_launch_log_reset()
    for args in ((None, one, one, one, one), (C.byref(params()), None, one, one, one), (C.byref(params()), one, None, one, one),
                 (C.byref(params()), one, one, None, one), (C.byref(params()), one, one, one, None)):      # (the fused next conv1 needs y1_next)
        assert L.dir_bottleneck_block_forward(*args, 2, 16, 16, None) == -1 and b'null pointer' in L.dir_last_error()
    assert L.dir_bottleneck_block_forward(C.byref(params(wstream=None)), one, one, one, one, 2, 16, 16, None) == -1 and b'missing parameters' in L.dir_last_error()
    assert L.dir_bottleneck_block_forward(C.byref(params(scale1n=None)), one, one, one, one, 2, 16, 16, None) == -1 and b'null pointer' in L.dir_last_error()
    assert L.dir_launch_log_get(C.create_string_buffer(64), 64) == 0


def test_stream_layout_is_the_documented_one():
    g = torch.Generator().manual_seed(5)
    w2 = torch.randn(256, 3, 3, 256, generator=g).to(torch.bfloat16)         # [Cout][ky][kx][Cin], as ConvOp keeps it
    w3 = torch.randn(1024, 256, generator=g).to(torch.bfloat16)
    w1n = torch.randn(256, 1024, generator=g).to(torch.bfloat16)
    lane = torch.arange(64)
    l32, h = lane & 31, lane >> 5
    e = torch.arange(8)
    for nxt in (w1n, None):
        s = packing.pack_l3_stream(w2, w3, nxt)
        ncf = 32 if nxt is not None else 0
        assert s.shape == (8, 144 + 2 * (32 + ncf), 64, 8) and s.dtype == torch.bfloat16 and s.is_contiguous()
        for w in (0, 3, 7):
            for f in (0, 1, 5, 36, 37, 75, 143):                               # conv2: step = slab * 9 + tap, ks
                step, ks = f // 4, f % 4
                slab, tap = step // 9, step % 9
                want = w2[(32 * w + l32)[:, None], tap // 3, tap % 3, (64 * slab + 8 * ks + 32 * h)[:, None] + e]
                assert torch.equal(s[w, f], want), (w, f)
            for half in (0, 1):
                base = 144 + half * (32 + ncf)
                for f in (0, 7, 15, 16, 22, 31):                               # conv3: channel block cb, k-step ks
                    cb, ks = f // 16, f % 16
                    k0 = 16 * ks + 8 * h if nxt is not None else 64 * (ks // 4) + 8 * (ks % 4) + 32 * h
                    want = w3[(half * 512 + 64 * w + 32 * cb + l32)[:, None], k0[:, None] + e]
                    assert torch.equal(s[w, base + f], want), (w, half, f)
                for fc in ((0, 9, 31) if nxt is not None else ()):             # next conv1
                    want = w1n[(32 * w + l32)[:, None], (half * 512 + 16 * fc + 8 * h)[:, None] + e]
                    assert torch.equal(s[w, base + 32 + fc], want), (w, half, fc)
