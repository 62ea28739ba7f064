"""dir_amd/packing.py: the weight streams of the activation-stationary and the streaming 1x1 kernels, element by element against plain loops
over the layout their docstrings (and include/dir_hip.h) state; and the engine's per-thread state.  Host only: nothing runs on a device."""
import functools
import threading

import numpy as np
import pytest
import torch

from dir_amd import engine as E
from dir_amd import packing


@functools.lru_cache(maxsize=None)
def _as_index(N, kh, kw, Cin, A):
    """flat index into W [Cout][kh][kw][Cin] of every element of [Cout / (128 A)][4 waves][kh kw Cin / 64 steps][4 k-steps][A][64 lanes][8]:
    step = (64-channel slab) * (kh kw) + tap; lanes 0-31 hold channels 8 ks .. + 8 of the slab, lanes 32-63 channels 32 + 8 ks .. + 8;
    a wave's A blocks of 32 output channels are consecutive, a workgroup's 4 waves cover 128 A output channels"""
    nt = kh * kw
    idx = np.empty((N // (128 * A), 4, nt * Cin // 64, 4, A, 64, 8), np.int64)
    for g in range(N // (128 * A)):
        for wv in range(4):
            for st in range(nt * Cin // 64):
                slab, tap = st // nt, st % nt
                for ks in range(4):
                    for cb in range(A):
                        for lane in range(64):
                            row = g * 128 * A + (wv * A + cb) * 32 + (lane & 31)
                            for e in range(8):
                                ch = 64 * slab + 8 * ks + 32 * (lane >> 5) + e
                                idx[g, wv, st, ks, cb, lane, e] = ((row * kh + tap // kw) * kw + tap % kw) * Cin + ch
    return idx


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _weights(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dtype)


@pytest.mark.parametrize('k,cin,cout,A', [(1, 64, 128, 1), (3, 64, 256, 2), (1, 128, 256, 2)])
def test_pack_as_weights_matches_the_stated_layout(k, cin, cout, A):
    w = _weights((cout, k, k, cin), torch.bfloat16, 1)
    got = packing.pack_as_weights(w, A)
    idx = _as_index(cout, k, k, cin, A)
    assert got.dtype == w.dtype and tuple(got.shape) == idx.shape and got.is_contiguous()
    assert np.unique(idx).size == w.numel()                       # a permutation: every weight exactly once
    np.testing.assert_array_equal(_bits(got), _bits(w).reshape(-1)[idx])
    assert E.pack_as_weights is packing.pack_as_weights           # the engine re-exports it


@pytest.mark.parametrize('n,k', [(128, 64), (256, 128), (384, 192)])
@pytest.mark.parametrize('src', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_pack_stream_weights_matches_the_stated_layout(n, k, src, dtype):
    """[Cout / NWG][4 waves][K / 64][4 k-steps][NCB][64 lanes][8] with NWG = 128 NCB, NCB = 2 where Cout is a multiple of 256: the loops above
    with a single tap; the values are the input's rounded to `dtype`"""
    w = _weights((n, k), src, 2)
    got = packing.pack_stream_weights(w, dtype=dtype)
    ncb = 2 if n % 256 == 0 else 1
    idx = _as_index(n, 1, 1, k, ncb)
    assert got.dtype == dtype and tuple(got.shape) == idx.shape and got.is_contiguous()
    np.testing.assert_array_equal(_bits(got), _bits(w.to(dtype)).reshape(-1)[idx])
    assert E.pack_stream_weights is packing.pack_stream_weights and E.pack_tail_stream is packing.pack_tail_stream


DEFAULTS = dict(variant=None, arith=None, capture=None, capture_fused=None, calibrating=False, no_out_split=False)


def _in_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    return out[0]


def test_thread_state_defaults_and_isolation():
    read = lambda: {k: getattr(E._TLS, k) for k in DEFAULTS}      # noqa: E731  (plain attribute reads: nothing has been set on the thread)
    assert _in_thread(read) == DEFAULTS
    before = read()

    def setter():
        E._TLS.variant, E._TLS.arith, E._TLS.calibrating, E._TLS.no_out_split = 21, 'f16x3', True, True
        E._TLS.capture, E._TLS.capture_fused = [], []
        return read()
    seen = _in_thread(setter)
    assert seen == dict(variant=21, arith='f16x3', capture=[], capture_fused=[], calibrating=True, no_out_split=True)
    assert _in_thread(read) == DEFAULTS                           # another thread, afterwards: untouched
    assert read() == before                                       # and so is this one
