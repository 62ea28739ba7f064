"""Execution plan of DIR.forward (eval) on MI355X, host side.  Everything is imported from here (`from dir_amd import engine as E`);
the modules behind it:

    common    per-thread switches (_TLS), dtype codes, variant constants, BatchNorm folding
    conv      ConvOp, DualConvOp, the stem's convolution
    backbone  the fused bottleneck launches and the ResNet-50 plan (BackboneOp)
    hrnet     the HRNet-W48 plan (HRNetOp)
    decoder   ResidualOp, ConvChainOp
    stage     token / MANO packers, StageOp, run_mano_pair
    autotune  TunedPlan: the autotuners and the tuning tables, inherited by DirEngine
    plan      DirEngine: packing and the kernel sequence of one forward
    pipeline  ForwardPipeline: several captured forwards in flight
"""
from .. import _capi                                                                                                  # noqa: F401
from .._capi import CONV_PRE_RELU, CONV_RELU, DT_BF16, DT_F16, DT_F16X1, DT_F16X1P, DT_F16X3, DT_F16X3P, DT_F32, ConvDesc      # noqa: F401
from ..packing import pack_as_weights, pack_l3_stream, pack_stream_weights, pack_tail_stream      # noqa: F401  (re-exported: tests and tools take them from here)
from .common import (AS_VARIANTS, F32, HALF, IMAGENET_MEAN, IMAGENET_STD, STREAM32_VARIANT, STREAM64_VARIANT, STREAM_VARIANT,      # noqa: F401
                     STREAM_VARIANTS, STREAMP_VARIANT, _TLS, _ann, _dt, _packing_arith, _pow2_scale, _ThreadState, _tok_wdt, _variant_for, bn_fold)
from .conv import ConvOp, DualConvOp, stem_conv_op                                                                    # noqa: F401
from .backbone import BackboneOp, BneckBlockOp, BneckChainOp, BneckTailOp, backbone_standalone                        # noqa: F401
from .hrnet import HRNetOp, _pad_conv_bn, _padc, hrnet_standalone                                                     # noqa: F401
from .decoder import ConvChainOp, ResidualOp                                                                          # noqa: F401
from .stage import StageOp, _pad_rows, pack_mano, pack_pgcn, pack_ste, pack_token_mlp, run_mano_pair                  # noqa: F401
from .autotune import TunedPlan                                                                                       # noqa: F401
from .plan import DirEngine                                                                                           # noqa: F401
from .pipeline import ForwardPipeline                                                                                 # noqa: F401
