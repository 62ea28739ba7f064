"""The convolution launches: ConvOp (one dir_conv2d_forward and its alternatives), DualConvOp (conv3 + projection shortcut), the stem's 4x4 form."""
import math
import os

import torch

from .. import _capi
from .._capi import CONV_PRE_RELU, CONV_RELU, DT_F16X1, DT_F16X1P, DT_F16X3, DT_F16X3P, ConvDesc
from ..packing import pack_as_weights, pack_stream_weights
from .common import AS_VARIANTS, F32, HALF, STREAM_VARIANT, STREAM_VARIANTS, _TLS, _ann, _dt, _packing_arith, _pow2_scale, _variant_for


class ConvOp(object):
    """one dir_conv2d_forward call with packed parameters"""
    def __init__(self, w_oihw, dtype, stride=1, pad=0, scale=None, shift=None, relu=False, pre=None, pre_relu=False,
                 out_dtype=None, arith=None):
        self.w = w_oihw.detach().permute(0, 2, 3, 1).contiguous().to(dtype)
        self.cout, self.kh, self.kw, self.cin = self.w.shape
        self.stride, self.pad, self.dtype = stride, pad, dtype
        self.out_dtype = out_dtype or dtype
        self.arith = (arith or _packing_arith()) if dtype == torch.float32 else None
        self.in_code = DT_F16X3 if self.arith == 'f16x3' else DT_F16X1 if self.arith == 'f16' else _dt(dtype)
        self.in_scale = 1.0                # f16x3: power of two applied to the activations before the split (set_in_scale / DirEngine.calibrate)
        if self.arith in ('f16x3', 'f16'):  # fp32 tensors, f16 hi / lo split arithmetic ('f16': hi only): weights split + pre-scaled here, 1 / p_n into the scale
            from ..functional import pack_f16x3_weights
            self.w, scale = pack_f16x3_weights(self.w.reshape(self.cout, -1), scale)
            self.scale0 = scale.float().contiguous().clone()  # the epilogue scale at in_scale = 1 (a copy: set_in_scale overwrites self.scale in place)
        self.scale = None if scale is None else scale.float().contiguous()
        self.shift = None if shift is None else shift.float().contiguous()
        self.pre_scale, self.pre_shift = (None, None) if pre is None else (pre[0].contiguous(), pre[1].contiguous())
        self.flags = (CONV_RELU if relu else 0) | (CONV_PRE_RELU if pre_relu else 0)
        self.ho = self.wo = 0
        self.in_cs_override = None
        # f16 arithmetic modes: layers whose activations are worth splitting ONCE (dir_split_f16_forward) so that both operands go global ->
        # LDS by DMA: every 3x3 (each input pixel is read by 9 taps and by every output-channel tile) and the 1x1 layers with >= 4
        # output-channel tiles; the rest (HBM-bound 1x1 layers with one or two tiles) keep converting while staging.  DIR_PRESPLIT=0|1|2: never / rule / always
        self.presplit = self.arith is not None and (ConvOp.PRESPLIT == 2 or (ConvOp.PRESPLIT == 1 and (
            self.kh * self.kw >= 9 or (self.cout >= 512 and self.cin >= 128))))
        self.split_consumer = None                         # f16 arithmetic modes: the ONE convolution reading this op's whole output (link_split)
        self.alg_k = self.kh * self.kw * self.cin          # reduction length the reference computes (stem: 147)
        self.variant = {}                                  # batch size -> DIR_CONV_VARIANT code chosen by DirEngine.autotune
        self._w_as = {}                                    # A -> the activation-stationary kernel's weight stream (pack_as_weights), packed on first use
        # streaming alternative for the HBM-bound 1x1 layers (dir_conv1x1_stream_forward), taken when autotune prefers it
        self.w_stream = None
        if (dtype in HALF and self.out_dtype == dtype and self.kh == 1 and self.kw == 1 and stride == 1 and pad == 0
                and self.cin % 64 == 0 and self.cout % 128 == 0 and self.cin <= 2304):
            self.w_stream = pack_stream_weights(self.w.reshape(self.cout, self.cin), dtype)

    PRESPLIT = int(os.environ.get('DIR_PRESPLIT', '1'))
    OUT_SPLIT = os.environ.get('DIR_OUT_SPLIT', '1') != '0'      # producers write the next convolution's pre-split operand (link_split)

    def link_split(self, consumer):
        """f16 arithmetic modes: declare that `consumer` (a ConvOp without pre-activation) is the ONLY reader of this convolution's whole fp32
        output: the epilogue then writes that tensor directly as the consumer's pre-split operand (f16 hi | lo slabs times the consumer's
        in_scale -- the same bytes as fp32), and the consumer takes the two-operand DMA path without a dir_split_f16_forward pass."""
        if (self.arith is not None and isinstance(consumer, ConvOp) and consumer.arith == self.arith and consumer.pre_scale is None
                and consumer.in_cs_override is None and self.cout == consumer.cin and self.cout % 32 == 0 and self.out_dtype == F32):
            self.split_consumer = consumer

    def set_in_scale(self, s):
        """f16x3: multiply the activations by the power of two `s` before the hi / lo split; 1 / s goes into the epilogue scale (exact)"""
        assert self.arith in ('f16x3', 'f16') and s > 0 and math.frexp(s)[0] == 0.5
        self.in_scale = float(s)
        self.scale.copy_(self.scale0 / s)

    def _calibrate(self, xs):
        """DirEngine.calibrate: pick in_scale from this batch -- the largest |activation| the layer reads lands in [2^9, 2^10)"""
        amax = max(float(t.abs().max()) for t in xs)
        if self.pre_scale is not None:     # the split sees relu(x * ps + pb): bound it by |x| max * |ps| max + |pb| max
            amax = amax * float(self.pre_scale.abs().max()) + float(self.pre_shift.abs().max())
        self.set_in_scale(_pow2_scale(amax))

    def __call__(self, x, out=None, out_coff=0, in_coff=0, residual=None, res_coff=0, bbox=None, _replay_split=None):
        B, H, W, cbuf = x.shape
        x_arg, in_coff_arg = x, in_coff
        if self.arith is not None and _TLS.calibrating:
            self._calibrate([x[..., in_coff:in_coff + self.cin]] if self.in_cs_override is None else [x])
        ho = self.ho or (H + 2 * self.pad - self.kh) // self.stride + 1
        wo = self.wo or (W + 2 * self.pad - self.kw) // self.stride + 1
        out_given, residual_ok = out, True
        if out is None:
            out = torch.empty(B, ho, wo, self.cout, device=x.device, dtype=self.out_dtype)
        pre_scale, pre_shift, flags, in_code, in_cs = self.pre_scale, self.pre_shift, self.flags, self.in_code, self.in_cs_override or cbuf
        if getattr(x, '_dir_split', False):
            # the producer's epilogue already wrote this tensor as f16 hi | lo slabs scaled by OUR in_scale (link_split): straight to the DMA path
            assert in_coff == 0 and cbuf == self.cin and pre_scale is None and bbox is None
            in_code = DT_F16X1P if self.arith == 'f16' else DT_F16X3P
        elif self.presplit and self.in_cs_override is None and bbox is None:
            # the activations' hi | lo split (with in_scale and the pre-activation) as its own HBM-bound pass; the convolution then reads
            # both operands by DMA (DIR_DT_F16X3P / F16X1P)
            xs = torch.empty(B, H, W, self.cin, device=x.device, dtype=F32)
            _ann('split_f16', 0, 2 * xs.numel() * 4, 'M=%d C=%d fp32 -> f16 hi | lo' % (B * H * W, self.cin))
            _capi.check(_capi.lib().dir_split_f16_forward(_capi.ptr(x), _capi.ptr(xs), B * H * W, self.cin, cbuf, in_coff, _capi.ptr(pre_scale), _capi.ptr(pre_shift),
                                                          1 if (flags & CONV_PRE_RELU) else 0, self.in_scale, 1 if self.arith == 'f16' else 0, _capi.stream_ptr()),
                        'dir_split_f16_forward')
            x, in_cs, in_coff, pre_scale, pre_shift = xs, self.cin, 0, None, None
            flags &= ~CONV_PRE_RELU
            in_code = DT_F16X1P if self.arith == 'f16' else DT_F16X3P
        d = ConvDesc(B, H, W, self.cin, in_cs, in_coff, self.cout, out.shape[3], out_coff,
                     residual.shape[3] if residual is not None else 0, res_coff, self.kh, self.kw, self.stride, self.pad,
                     in_code, _dt(out.dtype), flags, self.ho, self.wo, self.in_scale)
        cons = self.split_consumer
        write_split = (cons is not None and out_given is None and residual_ok and not _TLS.calibrating
                       and not _TLS.no_out_split and ConvOp.OUT_SPLIT)
        if _replay_split is not None:
            write_split = _replay_split
        if _TLS.capture is not None:       # autotune_energy: this call, replayable (same output buffer, same hand-over format)
            _TLS.capture.append((self, (x_arg,), dict(out=out, out_coff=out_coff, in_coff=in_coff_arg, residual=residual, res_coff=res_coff, bbox=bbox,
                                                  _replay_split=write_split)))
        if write_split:      # the only reader is the next convolution: write its pre-split operand instead of fp32 (same bytes, no split pass)
            d.out_split_scale = -cons.in_scale if cons.arith == 'f16' else cons.in_scale
        v = _variant_for(self, B)
        d.flags |= (v & 0xff) << 8
        if _capi.PROFILE is not None:
            nbytes = (B * H * W * self.cin * x.element_size() + self.w.numel() * self.w.element_size()
                      + B * ho * wo * self.cout * out.element_size() * (2 if residual is not None else 1))
            _capi.annotate(family='conv', flops=2.0 * B * ho * wo * self.cout * self.alg_k, bytes=nbytes, op=self, flops_real=2.0 * B * ho * wo * self.cout * self.alg_k * getattr(self, 'alg_scale', 1.0),
                           dtype=self.arith or ('f32' if self.dtype == F32 else 'bf16'),        # (roofline class: f16 storage runs at the bf16 MFMA rate)
                           shape='M=%d N=%d K=%d k%dx%d s%d' % (B * ho * wo, self.cout, self.kh * self.kw * self.cin, self.kh,
                                                              self.kw, self.stride))
        if v in AS_VARIANTS and bbox is None and pre_scale is None and self.dtype in HALF and out.dtype == self.dtype and self.arith is None:
            A_, PB_ = AS_VARIANTS[v]
            if _capi.lib().dir_conv2d_as_supported(d, A_, PB_):
                was = self._w_as.get(A_)
                if was is None:
                    was = self._w_as[A_] = pack_as_weights(self.w, A_)
                d.flags &= 0xff
                _capi.check(_capi.lib().dir_conv2d_as_forward(d, _capi.ptr(x), _capi.ptr(was), _capi.ptr(self.scale), _capi.ptr(self.shift), _capi.ptr(residual),
                                                              _capi.ptr(out), A_, PB_, _capi.stream_ptr()), 'dir_conv2d_as_forward')
                return out
            d.flags &= 0xff                                    # does not apply to this layer: the library's heuristic, like every other variant
        if v in STREAM_VARIANTS and self.w_stream is not None and residual is None and bbox is None and out.dtype == self.dtype:
            d.flags = (d.flags & 0xff) | ((v & 0xff) << 8 if v != STREAM_VARIANT else 0)
            _capi.check(_capi.lib().dir_conv1x1_stream_forward(d, _capi.ptr(x), None, None, _capi.ptr(self.w_stream), _capi.ptr(self.scale),
                                                               _capi.ptr(self.shift), _capi.ptr(self.pre_scale), _capi.ptr(self.pre_shift),
                                                               _capi.ptr(out), _capi.stream_ptr()), 'dir_conv1x1_stream_forward')
            return out
        if bbox is not None:
            _capi.check(_capi.lib().dir_conv2d_sparse_forward(d, _capi.ptr(x), _capi.ptr(self.w), _capi.ptr(self.scale),
                                                              _capi.ptr(self.shift), _capi.ptr(residual), _capi.ptr(out),
                                                              _capi.ptr(bbox), _capi.stream_ptr()), 'dir_conv2d_sparse_forward')
        else:
            _capi.check(_capi.lib().dir_conv2d_forward(d, _capi.ptr(x), _capi.ptr(self.w), _capi.ptr(self.scale),
                                                       _capi.ptr(self.shift), _capi.ptr(pre_scale),
                                                       _capi.ptr(pre_shift), _capi.ptr(residual), _capi.ptr(out),
                                                       _capi.stream_ptr()), 'dir_conv2d_forward')
        if write_split:
            out._dir_split = True
        return out


class DualConvOp(object):
    """dir_conv2d_dual_forward: a bottleneck's conv3 + BN with the projection shortcut (downsample conv + BN, stride s) folded
    in as a second K range -- relu(bn3(conv3(y)) + bn_ds(conv_ds(x))) in one launch, the identity tensor never exists
    (models/backbone/resnet.py:117-119,137-140).  Both BatchNorm scales are multiplied into the weight rows."""
    def __init__(self, w3, s3, h3, wds, sds, hds, stride2, dtype, relu=True):
        self.relu = relu
        self.cout, self.cin = w3.shape[0], w3.shape[1]
        self.cin2, self.stride2, self.dtype = wds.shape[1], stride2, dtype
        w = torch.cat([w3.float().flatten(1) * s3.float()[:, None], wds.float().flatten(1) * sds.float()[:, None]], 1)
        self.w = w.contiguous().to(dtype)                                    # [Cout][Cin + Cin2]
        self.arith = _packing_arith() if dtype == torch.float32 else None
        self.scale = None
        if self.arith is not None:         # split-precision rows; their power-of-two prescale comes back out through a scale vector
            from ..functional import pack_f16x3_weights
            self.w, self.scale = pack_f16x3_weights(self.w)
            self.scale0 = self.scale.clone()
        self.in_scale = 1.0
        self.shift = (h3.float() + hds.float()).contiguous()
        self.kh = self.kw = self.stride = 1
        self.pre_scale = None
        self.variant = {}
        self.w_stream = None
        if dtype in HALF and self.cin % 64 == 0 and self.cin2 % 64 == 0 and self.cout % 128 == 0:
            self.w_stream = pack_stream_weights(self.w, dtype)

    set_in_scale = ConvOp.set_in_scale

    def __call__(self, y, x, out=None, out_coff=0, x_decimated=False):
        """x_decimated: x already holds only the pixels the stride-`stride2` shortcut reads ([B,H,W,Cin2] at y's resolution)"""
        B, H, W, cbuf = y.shape
        if self.arith is not None and _TLS.calibrating:
            ConvOp._calibrate(self, [y[..., :self.cin], x[..., :self.cin2]])
        if out is None:
            out = torch.empty(B, H, W, self.cout, device=y.device, dtype=self.dtype)
        if _TLS.capture is not None:
            _TLS.capture.append((self, (y, x), dict(out=out, out_coff=out_coff, x_decimated=x_decimated)))
        d = ConvDesc(B, H, W, self.cin, cbuf, 0, self.cout, out.shape[3], out_coff, 0, 0, 1, 1, 1, 0,
                     DT_F16X3 if self.arith == 'f16x3' else DT_F16X1 if self.arith == 'f16' else _dt(self.dtype), _dt(self.dtype),
                     CONV_RELU if self.relu else 0, 0, 0, self.in_scale)
        v = _variant_for(self, B)
        d.flags |= (v & 0xff) << 8
        d2 = _capi.ConvSrc2(x.shape[1], x.shape[2], self.cin2, x.shape[3], 0, 1 if x_decimated else self.stride2)
        if _capi.PROFILE is not None:
            es, m = y.element_size(), B * H * W
            _capi.annotate(family='conv', flops=2.0 * m * self.cout * (self.cin + self.cin2), op=self,
                           bytes=(m * self.cin + m * self.cin2 + self.w.numel() + m * self.cout) * es,
                           dtype=self.arith or ('f32' if self.dtype == F32 else 'bf16'),
                           shape='M=%d N=%d K=%d+%d dual s%d' % (m, self.cout, self.cin, self.cin2, self.stride2))
        if v in STREAM_VARIANTS and self.w_stream is not None:
            d.flags = (d.flags & 0xff) | ((v & 0xff) << 8 if v != STREAM_VARIANT else 0)
            _capi.check(_capi.lib().dir_conv1x1_stream_forward(d, _capi.ptr(y), d2, _capi.ptr(x), _capi.ptr(self.w_stream), None, _capi.ptr(self.shift),
                                                               None, None, _capi.ptr(out), _capi.stream_ptr()), 'dir_conv1x1_stream_forward')
            return out
        if self.scale is not None:
            _capi.check(_capi.lib().dir_conv2d_dual_scaled_forward(d, _capi.ptr(y), d2, _capi.ptr(x), _capi.ptr(self.w), _capi.ptr(self.scale),
                                                                   _capi.ptr(self.shift), _capi.ptr(out), _capi.stream_ptr()),
                        'dir_conv2d_dual_scaled_forward')
            return out
        _capi.check(_capi.lib().dir_conv2d_dual_forward(d, _capi.ptr(y), d2, _capi.ptr(x), _capi.ptr(self.w), _capi.ptr(self.shift),
                                                        _capi.ptr(out), _capi.stream_ptr()), 'dir_conv2d_dual_forward')
        return out


def stem_conv_op(w, scale, shift, dtype):
    """7x7/2 stem over 2x2 space-to-depth blocks (dir_stem_prep_s2d): a 4x4 stride-1 convolution whose K-slab is a block-row
    window of 4 blocks x 16 channels; w'[n][j*16 + (dy*2+dx)*4 + c][r] = w[n, c, 2r+dy-1, 2j+dx-1]   (w = conv1.weight [64,3,7,7])"""
    wp = torch.zeros(64, 64, 4, 1, device=w.device, dtype=F32)        # [Cout, Cin', kh, kw=1]
    for r in range(4):
        for dy in range(2):
            ky = 2 * r + dy - 1
            if not 0 <= ky <= 6:
                continue
            for j in range(4):
                for dx in range(2):
                    kx = 2 * j + dx - 1
                    if 0 <= kx <= 6:
                        c0 = j * 16 + (dy * 2 + dx) * 4
                        wp[:, c0:c0 + 3, r, 0] = w[:, :, ky, kx]
    op = ConvOp(wp, dtype, stride=1, pad=0, scale=scale, shift=shift, relu=True)
    op.ho = op.wo = 128
    op.in_cs_override = 16
    op.alg_k = 147
    return op
