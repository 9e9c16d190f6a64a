"""Autograd Functions over the gfx950 C-ABI (dmayolo._lib).  Activations are NHWC
(torch channels_last, logical NCHW shape) in the storage dtype (float32 parity / bfloat16
throughput); master weights, BN statistics and reductions are fp32.

Every forward/backward here launches hand-written HIP kernels; no ATen compute op sits on the
hot path (torch is used for allocation and the current stream only).

One module per concern, named after the csrc unit(s) it drives; each imports only from the ones before it:

    _base      tensor / layout helpers, the vector contract
    sinks      the gradient-sink protocol (stated in its docstring)
    timer      KernelTimer
    fp8        e4m3 operands and delayed scaling             conv.hip (fp8 entry points), bn.hip
    spd        SM / MP passes                                spd.hip
    conv       ConvBNActFn and the conv engine               conv.hip conv_wgrad.hip dwconv.hip bwd1x1.hip bn.hip
    convmix    ConvActBNFn                                   convmix.hip
    pool       pools, resize, concat, add                    eltwise.hip
    attention  SCConv gate, CoorAttention, CBAM              eltwise.hip bn.hip (dmy_scgate_bn_*)
    image      image -> stem input                           eltwise.hip tta.hip
    swin       LayerNorm, attention, dropout, flatten        swin.hip mha.hip tal.hip
    adapt      adaptive-fusion necks                         adapt.hip
    hor        GnConv / HorBlock                             hor.hip

This file only re-exports: `dmayolo.functional.X` is the object its module defines, for every name the single-file
module had (the imported modules among them).  The mutable switches (DETERMINISTIC, DEFER_AFFINE, BWD1X1, PARAM_GEN,
F8_DELAYED, F8_HEADROOM) are one-element lists shared by identity: set them as `X[0] = value`, never rebind them.
"""
# flake8: noqa  (re-exports only)
import os
import weakref
from collections import namedtuple

import torch

from .. import _lib
from .._lib import call, ptr, stream, ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_SIGMOID, ACT_GELU, ACT_RELU, ACT_LEAKY
from ._base import DT, CL, VW, _CONST, dcode, pixel_stride, new_act, f32, const_vec, out_view, out_or_new, \
    concat_buffer, vec_ok, vec_check, vec_view, vec_pad, zero_padded_channels, conv_out_hw, even_hw, ctypes_off
from .sinks import GradSink, SliceSink, _SlicePart, SplitFn, sink_target, sink_result, pass_or_self, _write_target
from .timer import KernelTimer
from .fp8 import F8_DELAYED, F8_HEADROOM, F8Emit, _F8_WS, _f8_ws, fp8_eligible, _fp8_weight, _fp8_operands, _conv_fp8
from .spd import MaxPool2Fn, SpdSplitFn, SpaceToDepthFn, _spd_shape
from .conv import WGRAD_OIHW, WGRAD_ZEROED, DETERMINISTIC, DEFER_AFFINE, BWD1X1, PARAM_GEN, set_deterministic, \
    ConvGeom, WgradArena, WeightPrep, ConvSpec, BnLink, _SPECS, _PSPECS, spec_for, _param_spec, drop_specs, set_fp8, \
    f8_saturation, prep_weight, eval_coef, ConvBNActFn, conv_bn_act, _wgrad, _launch_conv_fwd, _launch_dw_fwd, \
    _dw_unsupported, _dw_check, _dw_operands, _fold_partials, _conv_operands, _conv_infer, _conv_infer_spd, \
    _conv_bn_stats, _bn_sync, _sync_slab, _bn_finalize, _bn_bwd_finalize, _defer_affine, _act_pass, _save_ctx, \
    _pgrad, _wgrad_target, _bn_bwd_coef, _bwd1x1, _dw_bias_in_wgrad, _act_bias_bwd, _dgrad, _conv_wgrad
from .convmix import ConvActBNFn, conv_act_bn, _actbn_stats, _actbn_infer
from .pool import MaxPoolFn, maxpool_chain3, AvgPoolFn, ResizeFn, ConcatFn, _inplace_concat, AddFn
from .attention import SCGateFn, CAPoolFn, CAApplyFn, GPoolFn, HalvesSigmoidFn, CBAMInFn, PixScaleFn
from .image import _image_src, image_s2d, tta_image, ToNHWC
from .swin import LayerNormFn, WinAttnFn, MHAFn, _DROP_STATE, _seed, DropoutFn, _sample_major, SampleScaleFn, \
    DropPathAddFn, FlattenLevelsFn
from .adapt import _lv3, AdaptGateFn, AdaptAddFn
from .hor import GateMulFn, LayerScaleAddFn
