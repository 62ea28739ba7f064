"""The decoder's fused launches: the hourglass Residual block (ResidualOp) and a 3x3 chained with the 1x1 that alone reads it (ConvChainOp)."""
import ctypes as C
import os

import torch

from .. import _capi
from .._capi import CONV_RELU, ConvDesc
from ..packing import pack_as_weights
from .common import F32, HALF, _TLS, _dt, bn_fold
from .conv import ConvOp, DualConvOp


class ResidualOp(object):
    """hourglass.Residual (models/backbone/hourglass.py:33-70), all convs carry a bias"""

    def __init__(self, sd, p, dtype):
        w = lambda k: sd['%s.%s.conv.weight' % (p, k)]  # noqa: E731
        b = lambda k: sd['%s.%s.conv.bias' % (p, k)]  # noqa: E731
        s2, h2 = bn_fold(sd, p + '.bn2', b('conv1'))
        self.c1 = ConvOp(w('conv1'), dtype, scale=s2, shift=h2, relu=True, pre=bn_fold(sd, p + '.bn1'), pre_relu=True)
        s3, h3 = bn_fold(sd, p + '.bn3', b('conv2'))
        self.c2 = ConvOp(w('conv2'), dtype, pad=1, scale=s3, shift=h3, relu=True)
        self.c3 = ConvOp(w('conv3'), dtype, shift=b('conv3'))
        # out = conv3(h) + skip_layer(x): the 1x1 skip projection is a second K range of conv3 (dir_conv2d_dual_forward); blocks whose input
        # and output widths are equal add x itself (hourglass.py:49-52)
        self.dual = None
        if w('skip_layer').shape[0] != w('skip_layer').shape[1]:
            one = torch.ones(w('conv3').shape[0], device=w('conv3').device)
            self.dual = DualConvOp(w('conv3'), one, b('conv3'), w('skip_layer'), one, b('skip_layer'), 1, dtype, relu=False)
        self.c1.link_split(self.c2)
        if self.dual is None:
            self.c2.link_split(self.c3)
        # the whole block as ONE launch (dir_residual_chain_forward) where the library has the shape: the three weight matrices as the kernel's
        # fragment streams, packed here once (eagerly: nothing is allocated or copied on the first call, which may be under graph capture)
        self.chain = None
        self.cout, self.cin, self.kh, self.kw, self.stride = self.c3.cout, self.c1.cin, 3, 3, 1      # what autotune / export_tuning read from a conv op
        self.variant = {}                                     # (a single kernel: every variant code is a no-op, as for BneckChainOp)
        if (self.res_chain and dtype in HALF and self.dual is not None and self.dual.w_stream is not None
                and _capi.lib().dir_residual_chain_supported(_dt(dtype), self.c1.cin, self.c1.cout, self.dual.cout, 1, 32, 32, self.c1.cin, 0, self.dual.cout, 0)):
            self.chain_w = (pack_as_weights(self.c1.w, 1), pack_as_weights(self.c2.w, 1),
                            pack_as_weights(self.dual.w.reshape(self.dual.cout, 1, 1, self.dual.cin + self.dual.cin2), 1))
            self.chain = _capi.ResChainParams(*([_capi.ptr(t) for t in self.chain_w] + [_capi.ptr(t) for t in (
                self.c1.pre_scale, self.c1.pre_shift, self.c1.scale, self.c1.shift, self.c2.scale, self.c2.shift, self.dual.shift)]
                + [self.c1.cin, self.c1.cout, self.dual.cout, _dt(dtype)]))

    res_chain = os.environ.get('DIR_RES_CHAIN', '1') != '0'        # 16-bit storage, 512 -> 128 -> 256 blocks on 32x32 / 16x16 maps: one launch per block

    def _chain_call(self, x, out=None, out_coff=0):
        """the fused launch, or None when the library does not take these shapes (the caller runs the three launches)"""
        B, H, W, cbuf = x.shape
        cs = out.shape[3] if out is not None else self.cout
        if x.dtype != self.c1.dtype or (out is not None and out.dtype != x.dtype) or not x.is_contiguous() or (out is not None and not out.is_contiguous()):
            return None
        if not _capi.lib().dir_residual_chain_supported(_dt(x.dtype), self.cin, self.c1.cout, self.cout, B, H, W, cbuf, 0, cs, out_coff):
            return None
        if out is None:
            out = torch.empty(B, H, W, self.cout, device=x.device, dtype=x.dtype)
        if _TLS.capture is not None:       # autotune_energy: this call, replayable
            _TLS.capture.append((self, (x,), dict(out=out, out_coff=out_coff)))
        if _capi.PROFILE is not None:
            m, mid = B * H * W, self.c1.cout
            _capi.annotate(family='conv', flops=2.0 * m * (mid * self.cin + mid * 9 * mid + self.cout * (mid + self.cin)), op=self, dtype='bf16',
                           shape='M=%d residual 1x1(%d->%d)+3x3+1x1(->%d)+skip' % (m, self.cin, mid, self.cout),
                           bytes=(m * (self.cin + self.cout) + self.c1.w.numel() + self.c2.w.numel() + self.dual.w.numel()) * 2)
        _capi.check(_capi.lib().dir_residual_chain_forward(C.byref(self.chain), _capi.ptr(x), _capi.ptr(out), B, H, W, cbuf, 0, cs, out_coff,
                                                           _capi.stream_ptr()), 'dir_residual_chain_forward')
        return out

    def __call__(self, x, out=None, out_coff=0):
        if self.chain is not None and self.res_chain:
            y = self._chain_call(x, out, out_coff)
            if y is not None:
                return y
        if self.dual is not None:
            return self.dual(self.c2(self.c1(x)), x, out=out, out_coff=out_coff)
        return self.c3(self.c2(self.c1(x)), out=out, out_coff=out_coff, residual=x)


class ConvChainOp(object):
    """a 3x3 ConvOp on the 32x32 map and the 1x1 ConvOp that is its ONLY reader as one launch (conv_as.hip's chained mode,
    dir_conv2d_as_chain_forward): models/dir.py:474-476 conv_final.0 -> conv_final.3 and models/dir.py:425-433 the merged seg | dense 3x3 -> their
    1x1s.  The 3x3's map never reaches memory; bit-identical to the two launches.  16-bit storage modes only: everything else (and
    DIR_HEAD_CHAIN=0) runs c1(c3(x)) as before.  For the tuning tables the pair stays TWO layers: the launch's profile record carries
    op = the 3x3 and covers = (the 1x1,), and DirEngine expands it (a chained 3x3's variant code is a no-op, the covered row's is carried)."""

    head_chain = os.environ.get('DIR_HEAD_CHAIN', '1') != '0'      # the A/B and test handle, as ResidualOp.res_chain

    def __init__(self, c3, c1):
        self.c3, self.c1 = c3, c1
        self.cout, self.cin, self.kh, self.kw, self.stride = c3.cout, c3.cin, c3.kh, c3.kw, c3.stride      # what autotune_energy reads from a captured op
        self.variant = c3.variant                              # (the 3x3's row)
        self.w = None
        f32_out = c1.out_dtype == F32
        if (c3.dtype in HALF and c1.dtype == c3.dtype and c3.arith is None and c3.pre_scale is None and c1.pre_scale is None and (c1.flags & ~CONV_RELU) == 0
                and (c1.kh, c1.kw, c1.stride, c1.pad, c1.cin) == (1, 1, 1, 0, c3.cout) and (f32_out or c1.out_dtype == c3.dtype)
                and _capi.lib().dir_conv2d_as_chain_supported(self._desc(1, 32, 32, c3.cin), c1.cout, _dt(c1.out_dtype))):
            # both weight streams packed here, eagerly: nothing is allocated or copied on the first call, which may be under graph capture
            w1 = c3._w_as.setdefault(2, pack_as_weights(c3.w, 2))
            if f32_out:                                        # <= 8 channels: zero rows up to one 128-channel slice of an A = 1 stream
                wp = torch.zeros(128, 1, 1, c1.cin, device=c1.w.device, dtype=c1.w.dtype)
                wp[:c1.cout] = c1.w
                self.w = (w1, pack_as_weights(wp, 1))
            else:
                self.w = (w1, pack_as_weights(c1.w, 2))

    def _desc(self, B, H, W, cbuf):
        c3 = self.c3
        return ConvDesc(B, H, W, c3.cin, cbuf, 0, c3.cout, c3.cout, 0, 0, 0, 3, 3, c3.stride, c3.pad, _dt(c3.dtype), _dt(c3.dtype), c3.flags & CONV_RELU, 0, 0, 1.0)

    def __call__(self, x, out=None):
        c3, c1 = self.c3, self.c1
        B, H, W, cbuf = x.shape
        if (self.w is None or not self.head_chain or x.dtype != c3.dtype or not x.is_contiguous() or _TLS.calibrating
                or (out is not None and (out.dtype != c1.out_dtype or out.shape != (B, H, W, c1.cout) or not out.is_contiguous()))):
            return c1(c3(x), out=out)
        d = self._desc(B, H, W, cbuf)
        if not _capi.lib().dir_conv2d_as_chain_supported(d, c1.cout, _dt(c1.out_dtype)):
            return c1(c3(x), out=out)
        if out is None:
            out = torch.empty(B, H, W, c1.cout, device=x.device, dtype=c1.out_dtype)
        if _TLS.capture is not None:       # autotune_energy: this call, replayable
            _TLS.capture.append((self, (x,), dict(out=out)))
        if _capi.PROFILE is not None:
            m = B * H * W
            _capi.annotate(family='conv', flops=2.0 * m * (c3.cout * c3.alg_k + c1.cout * c1.alg_k), op=c3, covers=(c1,), dtype='bf16',
                           shape='M=%d N=%d K=%d k3x3 s1 + 1x1 -> %d' % (m, c3.cout, c3.alg_k, c1.cout),
                           bytes=m * c3.cin * x.element_size() + (c3.w.numel() + c1.w.numel()) * c3.w.element_size() + m * c1.cout * out.element_size())
        _capi.check(_capi.lib().dir_conv2d_as_chain_forward(d, _capi.ptr(x), _capi.ptr(self.w[0]), _capi.ptr(c3.scale), _capi.ptr(c3.shift),
                                                            _capi.ptr(self.w[1]), _capi.ptr(c1.scale), _capi.ptr(c1.shift), c1.cout, 1 if c1.flags & CONV_RELU else 0,
                                                            _capi.ptr(out), c1.cout, 0, _dt(c1.out_dtype), _capi.stream_ptr()), 'dir_conv2d_as_chain_forward')
        return out
