"""What every module of the plan shares: the per-thread switches, the dtype codes, the variant constants, BatchNorm folding."""
import ctypes as C
import math
import threading

import torch

from .. import _capi
from .._capi import DT_BF16, DT_F16, DT_F32

F32 = torch.float32
IMAGENET_MEAN = (C.c_float * 3)(0.485, 0.456, 0.406)      # apps/eval.py:49-50
IMAGENET_STD = (C.c_float * 3)(0.229, 0.224, 0.225)
# Live per-launch measurement: set _capi.PROFILE to a list and every library call is bracketed by HIP events and recorded with the
# kernel names it launched plus the algorithmic work announced here with _capi.annotate() (bench.py roofline, DirEngine.autotune).
class _ThreadState(threading.local):
    """per-thread switches of the plan; the class attributes are what a thread sees before it sets anything"""
    variant = None          # DIR_CONV_VARIANT every conv of THIS thread is forced to (autotune); per thread, not global
    arith = None            # 'f16x3' | 'f16' while a DirEngine packs its parameters (_packing_arith)
    capture = None          # autotune_energy: list that collects every convolution call of a forward, replayable
    capture_fused = None    # tools/energy_profile.py: the same for the fused bottleneck launches
    calibrating = False     # DirEngine.calibrate: every f16-arithmetic convolution picks its in_scale from what it reads
    no_out_split = False    # forward(taps=...): the taps are read as fp32 maps, no pre-split hand-over


_TLS = _ThreadState()


def _variant_for(op, B):
    """DIR_CONV_VARIANT code of one launch of `op` at batch size B: the variant forced on this thread (autotune), else the op's tuned one"""
    return _TLS.variant if _TLS.variant is not None else op.variant.get(B, 0)


def _packing_arith():
    """'f16x3' while a DirEngine(dtype=float32, arith='f16x3') packs its parameters (per thread): every fp32 convolution built meanwhile
    takes the split-precision arithmetic (include/dir_hip.h: DIR_DT_F16X3), else None"""
    return _TLS.arith


def _ann(family, flops, nbytes, shape):
    """algorithmic work of the next library call (minimum HBM bytes = inputs + parameters + outputs once)"""
    if _capi.PROFILE is not None:
        _capi.annotate(family=family, flops=float(flops), bytes=float(nbytes), shape=shape)


HALF = (torch.bfloat16, torch.float16)      # the two 16-bit STORAGE kinds of the throughput modes: DIR_DT_BF16 | DIR_DT_F16 (round 5: f16 storage)


def _dt(dtype):
    return DT_F32 if dtype == torch.float32 else DT_F16 if dtype == torch.float16 else DT_BF16


def _tok_wdt(dtype):
    """weight dtype of the token path (P-GCN / STE Linears) for a feature-map dtype: the f16-storage mode keeps the bf16 weights (autocast
    semantics) -- its kernels take F32 | BF16, and the refined stages they feed are already inside 0.004 mm in the bf16 mode"""
    return torch.bfloat16 if dtype in HALF else torch.float32


def bn_fold(sd, prefix, conv_bias=None, eps=1e-5):
    """eval BatchNorm (after an optional conv bias) as y = x*scale + shift; folded in fp64."""
    g, b = sd[prefix + '.weight'].double(), sd[prefix + '.bias'].double()
    m, v = sd[prefix + '.running_mean'].double(), sd[prefix + '.running_var'].double()
    scale = g / torch.sqrt(v + eps)
    shift = b - m * scale
    if conv_bias is not None:
        shift = shift + conv_bias.double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


STREAM_VARIANT = 21      # DIR_CONV_VARIANT code: dir_conv1x1_stream_forward (1x1, bf16, Cout % 128 == 0), chosen per layer by autotune
STREAM64_VARIANT = 22    # the same kernel on 64-pixel workgroups (twice as many, half as long)
STREAM32_VARIANT = 23    # ... on 32-pixel workgroups (the 16x16 / 8x8 stages: 128-pixel tiles do not even cover the CUs there)
STREAMP_VARIANT = 24     # round 5: the pipelined form -- a fifth (producer) wave feeds a ring of activation chunks by LDS-DMA (no pre-activation form: those layers run 21)
STREAM_VARIANTS = (STREAM_VARIANT, STREAM64_VARIANT, STREAM32_VARIANT, STREAMP_VARIANT)
# round 6: the activation-stationary kernel for the small maps (conv_as.hip, dir_conv2d_as_forward): DIR_CONV_VARIANT -> (A = 32-channel blocks per
# wave, PB = 32-pixel blocks per workgroup).  Bit-identical to the tiled kernels (same K order and k-slots), so autotune may pick it per layer.
AS_VARIANTS = {25: (2, 2), 26: (2, 4), 27: (4, 2), 28: (1, 2)}


def _pow2_scale(amax):
    """f16 arithmetic modes: the power of two that puts the largest magnitude `amax` of a calibration batch into [2^9, 2^10) of the f16 range"""
    return 2.0 ** (10 - math.frexp(amax)[1]) if amax > 0 and math.isfinite(amax) else 1.0
