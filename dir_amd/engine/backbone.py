"""The ResNet-50 pyramid: the three fused bottleneck launches and the plan that chooses among them (BackboneOp)."""
import ctypes as C
import os

import torch

from .. import _capi
from .._capi import CONV_RELU
from ..packing import pack_l3_stream, pack_tail_stream
from .common import F32, HALF, IMAGENET_MEAN, IMAGENET_STD, _TLS, _ann, _dt, bn_fold
from .conv import ConvOp, DualConvOp, stem_conv_op


class BneckChainOp(object):
    """dir_bottleneck_chain_forward: conv2 + bn2 + ReLU + conv3 + bn3 + identity + ReLU of a layer1 bottleneck and, optionally,
    the next block's conv1 + bn1 + ReLU in one launch (models/backbone/resnet.py:122-140).  Built from the blocks' ConvOps;
    carries the attributes autotune / export_tuning read from a conv op (it has a single kernel: every variant code is a no-op)."""

    def __init__(self, c2, c3, c1n=None, dual=None):
        """c3: the block's conv3 ConvOp, or None with dual = DualConvOp (conv3 + projection shortcut, BN scales folded into rows)"""
        self.c2, self.c3, self.c1n, self.dual = c2, c3, c1n, dual
        self.cout, self.cin, self.kh, self.kw, self.stride = 256, c2.cin, 3, 3, 1
        self.variant = {}
        dev = c2.w.device
        if dual is None:
            self.w3 = c3.w.reshape(c3.cout, c3.cin).contiguous()
            self.wd, self.s3, self.h3 = None, c3.scale, c3.shift
        else:
            self.w3 = dual.w[:, :64].contiguous()
            self.wd = dual.w[:, 64:].contiguous()
            self.s3, self.h3 = torch.ones(256, device=dev, dtype=F32), dual.shift
        self.w1n = c1n.w.reshape(c1n.cout, c1n.cin).contiguous() if c1n is not None else None
        n = (lambda t: None) if c1n is None else _capi.ptr        # noqa: E731
        self.params = _capi.BneckChainParams(_capi.ptr(c2.w), _capi.ptr(c2.scale), _capi.ptr(c2.shift), _capi.ptr(self.w3),
                                             _capi.ptr(self.s3), _capi.ptr(self.h3), n(self.w1n),
                                             n(c1n.scale if c1n is not None else None), n(c1n.shift if c1n is not None else None),
                                             _capi.ptr(self.wd) if self.wd is not None else None, c1n.cout if c1n is not None else 0, 0, _dt(c2.dtype))

    @staticmethod
    def applies(c2, c3, c1n, dtype, dual=None):
        ok = dtype in HALF and c2.cin == 64 and c2.cout == 64 and c2.kh == 3 and c2.stride == 1 and c2.scale is not None
        if dual is None:
            ok = ok and c3.cin == 64 and c3.cout == 256 and c3.scale is not None
        else:
            ok = ok and dual.cin == 64 and dual.cin2 == 64 and dual.cout == 256 and dual.stride2 == 1 and dual.relu
        return ok and (c1n is None or (c1n.cin == 256 and c1n.cout in (64, 128) and c1n.kh == 1 and c1n.stride == 1 and c1n.scale is not None))

    def __call__(self, y1, x, decimate=False):
        """x: the block input -- the identity residual, or (dual) the projection shortcut's source.  decimate: write only the even (y, x)
        pixels of the block output, as [B,H/2,W/2,256] (the last layer1 block when nobody reads c1: dir_bneck_chain_params.out_decimate)"""
        residual, x2 = (None, x) if self.dual is not None else (x, None)
        B, H, W, _ = y1.shape
        if _TLS.capture_fused is not None:       # tools/energy_profile.py: replayable (allocates its own outputs)
            _TLS.capture_fused.append((self, (y1, x), dict(decimate=decimate)))
        self.params.out_decimate = 1 if decimate else 0
        out = torch.empty((B, H // 2, W // 2, 256) if decimate else (B, H, W, 256), device=y1.device, dtype=y1.dtype)
        y1n = torch.empty(B, H, W, self.c1n.cout, device=y1.device, dtype=y1.dtype) if self.c1n is not None else None
        if _capi.PROFILE is not None:
            m, nx = B * H * W, self.c1n is not None
            n2 = self.c1n.cout if nx else 0
            _capi.annotate(family='conv', flops=2.0 * m * (64 * 576 + 256 * 64 * (2 if x2 is not None else 1) + n2 * 256), op=self, dtype='bf16',
                           shape='M=%d chain 3x3(64)+1x1(256)%s' % (m, '+1x1(%d)' % n2 if nx else ''),
                           bytes=(m * (64 + 256 * (1 if residual is not None else 0) + (64 if decimate else 256) + n2 + (64 if x2 is not None else 0))
                                  + self.c2.w.numel() + self.w3.numel() * (2 if x2 is not None else 1) + (self.w1n.numel() if nx else 0)) * 2)
        _capi.check(_capi.lib().dir_bottleneck_chain_forward(C.byref(self.params), _capi.ptr(y1), _capi.ptr(residual), _capi.ptr(x2), _capi.ptr(out),
                                                             _capi.ptr(y1n), B, H, W, _capi.stream_ptr()), 'dir_bottleneck_chain_forward')
        return out, y1n


class BneckTailOp(object):
    """dir_bottleneck_tail_forward: conv3 + bn3 + identity + ReLU of a layer2 / layer3 bottleneck and the next block's conv1 + bn1 +
    ReLU in one launch (models/backbone/resnet.py:132-140,122-124): the block output is written once and not read back.  Built from
    the blocks' ConvOps; carries the attributes autotune / export_tuning read from a conv op (single kernel: variant codes are no-ops)."""
    GEOMETRIES = ((128, 128), (128, 256), (256, 256))

    def __init__(self, c3, c1n):
        self.c3, self.c1n = c3, c1n
        self.cout, self.cin, self.kh, self.kw, self.stride = c3.cout, c3.cin, 1, 1, 1
        self.variant = {}
        # the 8-wave stream (64-pixel tiles); the 4-wave "thin" kernel, slower at every size, is reached through functional.bottleneck_tail(waves=4)
        self.stream = pack_tail_stream(c3.w.reshape(c3.cout, c3.cin), c1n.w.reshape(c1n.cout, c1n.cin), 8, dtype=c3.dtype)
        self.params = _capi.BneckTailParams(_capi.ptr(self.stream), _capi.ptr(c3.scale), _capi.ptr(c3.shift), _capi.ptr(c1n.scale),
                                            _capi.ptr(c1n.shift), c3.cin, c1n.cout, 8, _dt(c3.dtype))

    @staticmethod
    def applies(c3, c1n, dtype):
        return (dtype in HALF and c3.kh == 1 and c3.stride == 1 and c3.scale is not None and c3.cout == 4 * c3.cin
                and c1n.kh == 1 and c1n.stride == 1 and c1n.cin == c3.cout and c1n.scale is not None and c1n.pre_scale is None
                and (c3.cin, c1n.cout) in BneckTailOp.GEOMETRIES)

    def __call__(self, y2, x):
        """y2: conv2's output [B,H,W,P]; x: the block input [B,H,W,4P] (identity residual) -> (block output, next y1)"""
        B, H, W, P = y2.shape
        M = B * H * W
        if _TLS.capture_fused is not None:
            _TLS.capture_fused.append((self, (y2, x), {}))
        out = torch.empty(B, H, W, self.c3.cout, device=y2.device, dtype=y2.dtype)
        y1n = torch.empty(B, H, W, self.c1n.cout, device=y2.device, dtype=y2.dtype)
        if _capi.PROFILE is not None:
            c4, n2 = self.c3.cout, self.c1n.cout
            _capi.annotate(family='conv', flops=2.0 * M * (P * c4 + c4 * n2), op=self, dtype='bf16',
                           shape='M=%d tail 1x1(%d->%d)+res+1x1(->%d)' % (M, P, c4, n2),
                           bytes=(M * (P + 2 * c4 + n2) + c4 * P + n2 * c4) * 2)
        _capi.check(_capi.lib().dir_bottleneck_tail_forward(C.byref(self.params), _capi.ptr(y2), _capi.ptr(x), _capi.ptr(out), _capi.ptr(y1n), M,
                                                            _capi.stream_ptr()), 'dir_bottleneck_tail_forward')
        return out, y1n


class BneckBlockOp(object):
    """dir_bottleneck_block_forward: conv2 + bn2 + ReLU + conv3 + bn3 + identity + ReLU of a layer3 identity bottleneck and, where c1n is
    given, the next block's conv1 + bn1 + ReLU in one launch (models/backbone/resnet.py:126-140,122-124): y2 stays on the CU.  Bit-identical
    to c2 followed by BneckTailOp (c1n given) or by c3 with the residual (c1n None).  For the tuning tables the launch stays the layers it
    replaces: its profile record carries op = c2 and covers = (`covered`,) -- the BneckTailOp or c3 that runs with DIR_L3_CHAIN=0."""

    def __init__(self, c2, c3, c1n=None, covered=None):
        self.c2, self.c3, self.c1n = c2, c3, c1n
        self.covers = (covered if covered is not None else c3,)
        self.cout, self.cin, self.kh, self.kw, self.stride = c3.cout, c2.cin, 3, 3, 1
        self.variant = c2.variant                              # (the 3x3's row; a single kernel: every variant code is a no-op)
        # the stream is packed here, eagerly: nothing is allocated or copied on the first call, which may be under graph capture
        self.stream = pack_l3_stream(c2.w, c3.w.reshape(c3.cout, c3.cin), None if c1n is None else c1n.w.reshape(c1n.cout, c1n.cin), dtype=c2.dtype)
        n = (lambda t: None) if c1n is None else _capi.ptr        # noqa: E731
        self.params = _capi.BneckBlockParams(_capi.ptr(self.stream), _capi.ptr(c2.scale), _capi.ptr(c2.shift), _capi.ptr(c3.scale), _capi.ptr(c3.shift),
                                             n(c1n.scale if c1n is not None else None), n(c1n.shift if c1n is not None else None),
                                             c2.cout, c1n.cout if c1n is not None else 0, _dt(c2.dtype))

    @staticmethod
    def applies(c2, c3, c1n, dtype):
        ok = (dtype in HALF and c2.arith is None and (c2.kh, c2.kw, c2.stride, c2.pad, c2.cin, c2.cout) == (3, 3, 1, 1, 256, 256)
              and c2.scale is not None and c2.pre_scale is None and (c2.flags & CONV_RELU)
              and (c3.kh, c3.stride, c3.cin, c3.cout) == (1, 1, 256, 1024) and c3.scale is not None and c3.pre_scale is None and (c3.flags & CONV_RELU))
        return bool(ok and (c1n is None or ((c1n.kh, c1n.stride, c1n.cin, c1n.cout) == (1, 1, 1024, 256) and c1n.scale is not None
                                            and c1n.pre_scale is None and (c1n.flags & CONV_RELU))))

    def supported(self, y1, x):
        B, H, W, Pn = y1.shape
        return bool(y1.dtype == self.c2.dtype and x.dtype == y1.dtype and y1.is_contiguous() and x.is_contiguous() and Pn == 256
                    and tuple(x.shape) == (B, H, W, 1024)
                    and _capi.lib().dir_bottleneck_block_supported(_dt(y1.dtype), 256, self.params.n_next, B, H, W))

    def __call__(self, y1, x):
        """y1: this block's conv1 output [B,H,16,256]; x: the block input [B,H,16,1024] (identity residual) -> (block output, next y1 | None)"""
        B, H, W, _ = y1.shape
        if _TLS.capture_fused is not None:
            _TLS.capture_fused.append((self, (y1, x), {}))
        out = torch.empty(B, H, W, 1024, device=y1.device, dtype=y1.dtype)
        y1n = torch.empty(B, H, W, 256, device=y1.device, dtype=y1.dtype) if self.c1n is not None else None
        if _capi.PROFILE is not None:
            m, n2 = B * H * W, self.params.n_next
            _capi.annotate(family='conv', flops=2.0 * m * (256 * 9 * 256 + 256 * 1024 + 1024 * n2), op=self.c2, covers=self.covers, dtype='bf16',
                           shape='M=%d block 3x3(256)+1x1(->1024)+res%s' % (m, '+1x1(->%d)' % n2 if n2 else ''),
                           bytes=(m * (256 + 2 * 1024 + n2) + 256 * 9 * 256 + 1024 * 256 + n2 * 1024) * 2)
        _capi.check(_capi.lib().dir_bottleneck_block_forward(C.byref(self.params), _capi.ptr(y1), _capi.ptr(x), _capi.ptr(out), _capi.ptr(y1n), B, H, W,
                                                             _capi.stream_ptr()), 'dir_bottleneck_block_forward')
        return out, y1n


class BackboneOp(object):
    """ResNet-50 pyramid (models/backbone/resnet.py:243-255): stem as a 4x4 implicit GEMM over 2x2 space-to-depth blocks,
    maxpool, 16 bottlenecks with BN folded into the conv epilogues, the residual add + ReLU fused, and the four projection
    shortcuts folded into their block's conv3 as a second K range (dir_conv2d_dual_forward)."""
    fused_stem = os.environ.get('DIR_FUSED_STEM', '1') != '0'       # bf16 mode: conv1 + bn1 + ReLU + maxpool in one launch
    bneck_chain = os.environ.get('DIR_BNECK_CHAIN', '1') != '0'     # bf16 mode, layer1: conv2 + conv3 (+ next conv1) in one launch
    bneck_tail = os.environ.get('DIR_BNECK_TAIL', '1') != '0'       # bf16 mode, layer2 / layer3: conv3 + residual + next conv1 in one launch
    l3_chain = os.environ.get('DIR_L3_CHAIN', '1') != '0'           # 16-bit storage, layer3 identity blocks: conv2 + conv3 (+ next conv1) in one launch

    def __init__(self, sd, p, dtype, device):
        dt = self.dtype = dtype
        self.device = device
        # dir_stem_pool_forward: conv1.weight [64,3,7,7] -> bf16 [64][ky 7][kx 8][c 4] (zero for kx = 7, c = 3)
        w = sd[p + '.conv1.weight']
        wk = torch.zeros(64, 7, 8, 4, device=w.device, dtype=F32)
        wk[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        self.stem_w = wk.to(dtype if dtype in HALF else torch.bfloat16).contiguous().to(device)
        s_, h_ = bn_fold(sd, p + '.bn1')
        self.stem_scale, self.stem_shift = s_.float().contiguous().to(device), h_.float().contiguous().to(device)
        self.stem = stem_conv_op(sd[p + '.conv1.weight'], s_, h_, dt)     # staged path (fp32 mode, DIR_FUSED_STEM=0)
        self.layers = []
        for li, n in enumerate((3, 4, 6, 3), start=1):
            blocks = []
            for b in range(n):
                q = '%s.layer%d.%d' % (p, li, b)
                stride = 2 if (b == 0 and li > 1) else 1
                s1, h1 = bn_fold(sd, q + '.bn1')
                s2, h2 = bn_fold(sd, q + '.bn2')
                s3, h3 = bn_fold(sd, q + '.bn3')
                blk = dict(c1=ConvOp(sd[q + '.conv1.weight'], dt, scale=s1, shift=h1, relu=True),
                           c2=ConvOp(sd[q + '.conv2.weight'], dt, stride=stride, pad=1, scale=s2, shift=h2, relu=True),
                           c3=ConvOp(sd[q + '.conv3.weight'], dt, scale=s3, shift=h3, relu=True))
                if (q + '.downsample.0.weight') in sd:
                    sd_, hd_ = bn_fold(sd, q + '.downsample.1')
                    blk['dual'] = DualConvOp(sd[q + '.conv3.weight'], s3, h3, sd[q + '.downsample.0.weight'], sd_, hd_, stride, dt)
                blk['c1'].link_split(blk['c2'])
                if 'dual' not in blk:
                    blk['c2'].link_split(blk['c3'])
                blocks.append(blk)
            self.layers.append(blocks)
        # layer1 (HBM-bound): blocks without a projection shortcut run conv2 -> conv3 -> (next block's conv1) as one kernel
        if self.bneck_chain:
            l1 = self.layers[0]
            for i, blk in enumerate(l1):
                nxt = l1[i + 1]['c1'] if i + 1 < len(l1) else self.layers[1][0]['c1']      # last block: layer2's first conv1
                if 'dual' in blk:
                    if BneckChainOp.applies(blk['c2'], None, nxt, dt, dual=blk['dual']):
                        blk['chain'] = BneckChainOp(blk['c2'], None, nxt, dual=blk['dual'])
                elif BneckChainOp.applies(blk['c2'], blk['c3'], nxt, dt):
                    blk['chain'] = BneckChainOp(blk['c2'], blk['c3'], nxt)

        # layer2 / layer3 (HBM- / latency-bound 1x1 convs): identity blocks hand their output to the next block's conv1 on chip
        if self.bneck_tail:
            for li in (1, 2):
                blocks = self.layers[li]
                for i, blk in enumerate(blocks):
                    if 'dual' in blk or 'chain' in blk:
                        continue
                    nxt = blocks[i + 1]['c1'] if i + 1 < len(blocks) else self.layers[li + 1][0]['c1']
                    if BneckTailOp.applies(blk['c3'], nxt, dt):
                        blk['tail'] = BneckTailOp(blk['c3'], nxt)

        # layer3's identity blocks from conv2 on as ONE launch each (dir_bottleneck_block_forward): the next conv1 rides along where the tail
        # launch it replaces had it (same k-slots), the layer's last block ends at its output
        if self.l3_chain:
            for i, blk in enumerate(self.layers[2]):
                if 'dual' in blk or 'chain' in blk:
                    continue
                nxt = blk['tail'].c1n if 'tail' in blk else None
                if BneckBlockOp.applies(blk['c2'], blk['c3'], nxt, dt):
                    blk['block'] = BneckBlockOp(blk['c2'], blk['c3'], nxt, covered=blk.get('tail'))

    def __call__(self, img):
        L, dt, dev = _capi.lib(), self.dtype, self.device
        B = img.shape[0]
        if self.fused_stem and dt in HALF:
            x = torch.empty(B, 64, 64, 64, device=dev, dtype=dt)
            u8 = img.dtype == torch.uint8
            _ann('stem', 2.0 * B * 128 * 128 * 64 * 147, img.numel() * img.element_size() + x.numel() * 2 + self.stem_w.numel() * 2,
                 'B=%d 7x7/2 conv + bn + relu + maxpool' % B)
            _capi.check(L.dir_stem_pool_forward_dt(_capi.ptr(img), 2 if u8 else 0, _dt(dt), IMAGENET_MEAN, IMAGENET_STD, _capi.ptr(self.stem_w),
                                                _capi.ptr(self.stem_scale), _capi.ptr(self.stem_shift), _capi.ptr(x), B, 256, 256,
                                                _capi.stream_ptr()), 'dir_stem_pool_forward_dt')
            return self._layers(x)
        Hs, Ws = 131, 132                                                        # blocks Y, X = 0 .. 130 (+1 column: even rows)
        xp = torch.empty(B, Hs, Ws, 16, device=dev, dtype=dt)
        _ann('stem', 0, img.numel() * img.element_size() + xp.numel() * xp.element_size(), 'B=%d space-to-depth staging' % B)
        if img.dtype == torch.uint8:     # [B,256,256,3] BGR as decoded: normalisation fused into the staging (apps/eval.py:59-61)
            _capi.check(L.dir_stem_prep_s2d_u8(_capi.ptr(img), _capi.ptr(xp), IMAGENET_MEAN, IMAGENET_STD, B, 256, 256, Hs, Ws,
                                               _dt(dt), _capi.stream_ptr()), 'dir_stem_prep_s2d_u8')
        else:
            _capi.check(L.dir_stem_prep_s2d(_capi.ptr(img), _capi.ptr(xp), B, 256, 256, Hs, Ws, _dt(dt), _capi.stream_ptr()),
                        'dir_stem_prep_s2d')
        s1 = self.stem(xp)                                                       # [B,128,128,64]
        x = torch.empty(B, 64, 64, 64, device=dev, dtype=dt)
        _ann('stem', 0, (s1.numel() + x.numel()) * x.element_size(), 'B=%d maxpool 3x3/2' % B)
        _capi.check(L.dir_maxpool3x3s2(_capi.ptr(s1), _capi.ptr(x), B, 128, 128, 64, _dt(dt), _capi.stream_ptr()),
                    'dir_maxpool3x3s2')
        return self._layers(x)

    decimate_c1 = os.environ.get('DIR_DECIMATE_C1', '1') != '0'     # bf16 mode: c1 is not produced unless asked for (taps / backbone_standalone)

    def _layers(self, x):
        """the four layers of the pyramid on the stem's output -> [c1, c2, c3, c4] (c1 None where it is not produced)"""
        feats = []
        y1 = None                                                    # the next block's conv1 output, where the previous launch already made it
        x_dec = False                                                # x holds only the even pixels of the previous layer's output (decimate_c1)
        for li, blocks in enumerate(self.layers):
            for bi, blk in enumerate(blocks):
                if 'chain' in blk:
                    # the last layer1 block's output is read by layer2's stride-2 projection shortcut only (its conv1 is fused into this launch):
                    # when nobody asks for c1, a quarter of its pixels are written (dir_bneck_chain_params.out_decimate)
                    dec = (self.decimate_c1 and li == 0 and bi == len(blocks) - 1 and blk['chain'].c1n is not None and 'dual' in self.layers[1][0]
                           and self.layers[1][0]['dual'].stride2 == 2 and 'chain' not in self.layers[1][0] and not _TLS.no_out_split)
                    x, y1 = blk['chain'](y1 if y1 is not None else blk['c1'](x), x, decimate=dec)
                    x_dec = dec
                    continue
                if 'block' in blk and self.l3_chain:
                    y1 = y1 if y1 is not None else blk['c1'](x)
                    if blk['block'].supported(y1, x):
                        x, y1 = blk['block'](y1, x)
                        continue
                if 'tail' in blk and (x.shape[0] * x.shape[1] * x.shape[2]) % 64 == 0:
                    x, y1 = blk['tail'](blk['c2'](y1 if y1 is not None else blk['c1'](x)), x)
                elif 'dual' in blk:                                  # conv3 + projection shortcut in one launch
                    x, y1 = blk['dual'](blk['c2'](y1 if y1 is not None else blk['c1'](x)), x, x_decimated=x_dec), None
                    x_dec = False
                else:
                    x, y1 = blk['c3'](blk['c2'](y1 if y1 is not None else blk['c1'](x)), residual=x), None
            feats.append(None if x_dec else x)                     # (c1 is not produced when its only reader is the strided shortcut)
        return feats


def backbone_standalone(module, x, compute_dtype=torch.float32):
    """ResNet.forward of the mirror module: NCHW float32 in, [c1..c4] NCHW float32 out."""
    _capi.require_cuda(x)
    if module.training:
        raise NotImplementedError('dir_amd implements the inference path (eval-mode BatchNorm); call .eval()')
    sd = {'b.' + k: v.detach() for k, v in module.state_dict().items()}
    op = BackboneOp(sd, 'b', compute_dtype, x.device)
    op.decimate_c1 = False                                           # ResNet.forward returns c1
    with torch.cuda.device(x.device):
        feats = op(_capi.f32c(x.detach()))
    return [f.permute(0, 3, 1, 2).float() for f in feats]
