"""Device side of tests/test_gpu_gemm_sweep.py and tests/test_gpu_wgrad_sweep.py: guarded buffers and the raw C ABI calls with their launch log."""
import ctypes as C

import numpy as np
import torch

from dir_amd import _capi

GUARD = 64                         # guard floats before and after every buffer (256 bytes: alignment kept)


class Buf(object):
    """a flat float32 array between two runs of GUARD guard floats, optionally 4 bytes off 16-byte alignment; guard floats hold `guard`"""
    def __init__(self, flat, mis=False, guard=float('nan')):
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        self.n, self.off = flat.size, GUARD + (1 if mis else 0)
        self.t = torch.full((2 * GUARD + 4 + self.n,), guard, device='cuda', dtype=torch.float32)
        self.t[self.off:self.off + self.n] = torch.from_numpy(flat).cuda()
        self.t0 = self.t.clone()

    def ptr(self, elem=0):
        return C.c_void_p(int(self.t.data_ptr() + 4 * (self.off + int(elem))))

    def body(self):
        return self.t[self.off:self.off + self.n]

    def get(self):
        return self.body().cpu().numpy()

    def unchanged(self):
        return torch.equal(self.t.view(torch.int32), self.t0.view(torch.int32))

    def untouched_outside(self, owned):
        """guard floats and every element of the body outside `owned` (flat indices) keep their bits"""
        chg = self.t.view(torch.int32) != self.t0.view(torch.int32)
        keep = torch.ones(self.n, dtype=torch.bool, device='cuda')
        keep[torch.from_numpy(np.asarray(owned, np.int64).reshape(-1)).cuda()] = False
        chg[self.off:self.off + self.n] &= keep
        return not bool(chg.any())


class Bytes(object):
    """a workspace of exactly n bytes between 256 guard bytes on either side, everything pre-filled with 0xFF"""
    def __init__(self, n):
        self.n = int(n)
        self.t = torch.full((512 + self.n,), 0xFF, device='cuda', dtype=torch.uint8)

    def ptr(self):
        return C.c_void_p(int(self.t.data_ptr() + 256))

    def guards_intact(self):
        return bool((self.t[:256] == 0xFF).all()) and bool((self.t[256 + self.n:] == 0xFF).all())

    def floats(self):
        return self.t[256:256 + self.n].view(torch.float32)


def call(name, *args, expect_ok=True):
    """one library call -> (return code, the kernels it launched)"""
    L = _capi.lib()
    L.dir_launch_log_reset()
    rc = getattr(L, name)(*args)
    if expect_ok:
        _capi.check(rc, name)
    buf = C.create_string_buffer(2048)
    L.dir_launch_log_get(buf, 2048)
    return rc, [s for s in buf.value.decode().split(',') if s]


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
