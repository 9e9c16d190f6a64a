"""Drop-in replacements for the reference's YAML modules (models/common.py, models/cspcm.py).

Same class names, constructor signatures, parameter/buffer names (state_dict keys) and the
attributes other reference code reads (`Conv.conv/.bn/.forward_fuse`, `AdConcat*.w`, real
nn.BatchNorm2d / nn.Conv2d instances for optimizer grouping and initialize_weights).
forward() runs the gfx950 kernels through dmayolo.functional; there is no CPU path.

Activation tensors are NHWC (torch.channels_last) in the model's storage dtype.
"""
import ctypes
import functools
import logging
import math
import os
import weakref
from copy import copy
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from .. import functional as Fn
from ..functional import ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_SIGMOID, ACT_GELU, ACT_RELU, ACT_LEAKY
from ..functional import call, ptr, stream
from ..utils.general import make_divisible, nms_padded, xyxy2xywh
from ..utils.torch_utils import time_sync

_LOG = logging.getLogger('dmayolo')

__all__ = ['autopad', 'Conv', 'DWConv', 'GhostConv', 'GhostBottleneck', 'C3Ghost', 'Bottleneck', 'C3', 'SPPF', 'SPPFCSPC', 'SCConv', 'CoorAttention', 'CA',
           'CABottleneck', 'C3CA', 'Concat', 'AdConcat2', 'AdConcat3', 'AdaptConcat', 'Adapt_Add2', 'Adapt_Add3', 'AdaptADD',
           'Upsample', 'C3STR', 'SwinTransformerBlock',
           'SwinTransformerLayer', 'WindowAttention', 'Mlp', 'DropPath', 'space_to_depth', 'SM', 'MP', 'DMConv', 'DMMConv',
           'DMMConv2', 'SPP', 'CBAM', 'LayerNorm', 'GnConv', 'HorBlock', 'C3HB', 'ConvMix', 'CSPCM',
           'ChannelAttentionModule', 'SpatialAttentionModule', 'C3TR', 'TransformerBlock', 'TransformerLayer']


def autopad(k, p=None):
    """models/common.py:33-48."""
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


def act_code(m):
    if m is None or isinstance(m, nn.Identity):
        return ACT_NONE
    if isinstance(m, nn.SiLU):
        return ACT_SILU
    if isinstance(m, nn.Hardswish):
        return ACT_HARDSWISH
    if isinstance(m, nn.Sigmoid):
        return ACT_SIGMOID
    if isinstance(m, nn.GELU):
        return ACT_GELU
    if isinstance(m, nn.ReLU):
        return ACT_RELU
    if isinstance(m, nn.LeakyReLU):
        if m.negative_slope != 0.1:
            raise NotImplementedError(f'LeakyReLU({m.negative_slope}) has no gfx950 kernel (only the slope 0.1 of '
                                      'add_conv, models/common.py:1080)')
        return ACT_LEAKY
    raise NotImplementedError(f'activation {type(m).__name__} has no gfx950 kernel')


def _pad_int(p):
    return p if isinstance(p, int) else p[0]


def conv_forward(conv, bn, act, x, res=None, xsink=None, rsink=None, out=None, defer=False):
    """conv (nn.Conv2d, dilation=1; groups 1, or depthwise: groups == channels) -> optional BN -> act (+ residual) on
    the HIP path.  Any other grouping raises NotImplementedError (functional._dw_operands).
    xsink / rsink: Fn.GradSink for the gradients of x / res when they have other consumers.  defer: a train-mode BN
    layer without activation returns its pre-BN output for a consumer that applies the BN itself (SCConv's gate)"""
    assert conv.dilation in (1, (1, 1)), 'dilated conv not on the DMA-YOLO path'
    s = conv.stride if isinstance(conv.stride, int) else conv.stride[0]
    pad, a = _pad_int(conv.padding), act_code(act)
    return Fn.conv_bn_act(x, conv.weight, conv.bias, bn, s, pad, a, res=res, spec=Fn.spec_for(conv, s, pad, a, bn),
                          xsink=xsink, rsink=rsink, out=out, defer=defer)


class Conv(nn.Module):
    """conv + BN + SiLU: models/cspcm.py:11-23 (YAML-level Conv) == models/common.py:50-77."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    def forward(self, x, res=None, xsink=None, rsink=None, out=None):
        return conv_forward(self.conv, self.bn, self.act, x, res, xsink, rsink, out)

    def forward_fuse(self, x, res=None, xsink=None, rsink=None, out=None):
        return conv_forward(self.conv, None, self.act, x, res, xsink, rsink, out)


class DWConv(Conv):
    """Depthwise conv + BN + act, models/common.py:79-82 (groups = gcd(c1, c2); the kernels take c1 == c2)."""

    def __init__(self, c1, c2, k=1, s=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act)


class GhostConv(nn.Module):
    """Ghost convolution, models/common.py:666-685: cat(y, cv2(y)) with y = cv1(x) and cv2 a 5x5 depthwise conv.
    One c2-channel NHWC buffer: cv1 writes the first half through out=, cv2 reads that slice (pixel stride c2) and
    writes the second half, so the concat copies nothing (as C3's in-place concat)."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act)

    def forward(self, x, xsink=None):
        """xsink: the caller's GradSink for x.  When cv1 has no separate activation pass (a fused linear layer) it
        returns its own tensor and ConcatFn copies the halves instead."""
        c_ = self.cv1.conv.out_channels
        c = self.cv1.conv
        OH, OW = Fn.conv_out_hw(x.shape[2], x.shape[3], c.kernel_size[0], c.stride[0], c.padding[0])
        cat = Fn.concat_buffer(x.shape[0], 2 * c_, OH, OW, x)
        # y -> cv2 and the concat.  The concat's contribution is a slice of the block's upstream gradient, which other
        # branches (GhostBottleneck's shortcut) still read: cv2's data-grad must not accumulate into it (adopt=False)
        sk = Fn.GradSink(2, adopt=False)
        y = self.cv1(x, xsink=xsink, out=cat[:, :c_])
        return Fn.ConcatFn.apply(None, 0.0, (sk, None), y, self.cv2(y, xsink=sk, out=cat[:, c_:]))


class GhostBottleneck(nn.Module):
    """models/common.py:687-699: conv = GhostConv -> (DWConv when s == 2, else the Identity placeholder) -> GhostConv
    (linear), plus the shortcut (DWConv -> Conv when s == 2, else identity), added with AddFn."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1),
                                  DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False),
                                      Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def forward(self, x):
        sk = Fn.GradSink(2)  # x -> conv[0].cv1 and the shortcut
        a = self.conv[0](x, xsink=sk)
        if not isinstance(self.conv[1], nn.Identity):
            a = self.conv[1](a)
        a = self.conv[2](a)
        if isinstance(self.shortcut, nn.Identity):
            return Fn.AddFn.apply(x, a, sk)
        return Fn.AddFn.apply(self.shortcut[1](self.shortcut[0](x, xsink=sk)), a, None)


class Bottleneck(nn.Module):
    """models/common.py:119-137; the residual add is fused into cv2's BN/act epilogue."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        if not self.add:
            return self.cv2(self.cv1(x), out=out)
        sk = Fn.GradSink(2)  # x -> cv1 and the residual
        return self.cv2(self.cv1(x, xsink=sk), res=x, rsink=sk, out=out)


# in-place C3 concat (C3.forward): 0 off (copy), 1 Bottleneck stacks, 2 also Swin blocks (C3STR); DMY_INPLACE_CAT
_INPLACE_CAT = int(os.environ.get('DMY_INPLACE_CAT', '2'))


# inference: C3's cv1 and cv2 (both 1x1 over x) as ONE conv with their weights / BN stacked; DMY_C3_PAIR (default on)
_C3_PAIR = os.environ.get('DMY_C3_PAIR', '1') == '1'
_PAIRS = weakref.WeakKeyDictionary()  # C3 module -> (source key, weight, bias, bn, act); not module state, so no
# state_dict / checkpoint entry


class _PairBN:
    """two eval-mode BatchNorm2d side by side (the stacked cv1 | cv2 of C3._pair), as conv_bn_act reads one"""
    training, track_running_stats, momentum = False, True, None

    def __init__(self, a, b):
        self.eps = a.eps
        self.weight, self.bias, self.running_mean, self.running_var = (
            torch.cat([getattr(a, n).detach(), getattr(b, n).detach()])
            for n in ('weight', 'bias', 'running_mean', 'running_var'))


class C3(nn.Module):
    """models/common.py:159-182."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    def _pair(self):
        """(weight, bias, bn, act) of cv1 | cv2 stacked along the output channels, rebuilt when a source parameter or
        BN buffer changes (torch _version / Fn.PARAM_GEN); None when the two layers cannot share a launch"""
        c1, c2 = self.cv1, self.cv2
        b1, b2 = getattr(c1, 'bn', None), getattr(c2, 'bn', None)
        w1, w2 = c1.conv.weight, c2.conv.weight
        if (b1 is None) != (b2 is None) or type(c1.act) is not type(c2.act) or w1.shape[1:] != w2.shape[1:] or \
                tuple(w1.shape[2:]) != (1, 1) or tuple(c1.conv.stride) != (1, 1) or tuple(c2.conv.stride) != (1, 1) or \
                (b1 is not None and (b1.eps != b2.eps or b1.training or b2.training)) or \
                (c1.conv.bias is None) != (c2.conv.bias is None):
            return None
        srcs = [w1, w2, c1.conv.bias, c2.conv.bias] + ([b1.weight, b1.bias, b1.running_mean, b1.running_var, b2.weight,
                                                        b2.bias, b2.running_mean, b2.running_var] if b1 is not None else [])
        key = (Fn.PARAM_GEN[0],) + tuple((t.data_ptr(), t._version) if t is not None else None for t in srcs)
        ent = _PAIRS.get(self)
        if ent is None or ent[0] != key:
            w = torch.cat([w1.detach(), w2.detach()])
            b = torch.cat([c1.conv.bias.detach(), c2.conv.bias.detach()]) if c1.conv.bias is not None else None
            ent = _PAIRS[self] = (key, w, b, _PairBN(b1, b2) if b1 is not None else None, act_code(c1.act))
        return ent[1:]

    def forward(self, x, out=None):
        """out: a concat_buffer slice cv3 writes the block's output into (Model's concat plan)"""
        blocks = list(self.m) if isinstance(self.m, nn.Sequential) else []
        seq = bool(blocks) and type(blocks[-1]) is Bottleneck and _INPLACE_CAT >= 1
        pair = self._pair() if seq and _C3_PAIR and not self.training and not torch.is_grad_enabled() else None
        if pair is not None:
            # inference: one 1x1 launch writes cv1's and cv2's activations into the two halves of the concat buffer;
            # the Bottleneck stack starts from the first half and its last block writes its output back over it (for
            # one block that is its own residual input: each output element is read as the residual, then written, by
            # the epilogue that owns it), so cv3 reads the buffer as the concat
            w, b, bn, act = pair
            c_ = w.shape[0] // 2
            cat = Fn.concat_buffer(x.shape[0], 2 * c_, x.shape[2], x.shape[3], x)
            Fn.conv_bn_act(x, w, b, bn, 1, 0, act, out=cat)
            a = cat[:, :c_]
            for blk in blocks[:-1]:
                a = blk(a)
            a = blocks[-1](a, out=cat[:, :c_])
            return self.cv3(Fn.ConcatFn.apply(None, 0.0, None, a, cat[:, c_:]), out=out)
        sk = Fn.GradSink(2)  # x -> cv1 and cv2
        a = self.cv1(x, xsink=sk)
        if not seq and not (getattr(self.m, 'dmy_out', False) and _INPLACE_CAT >= 2):
            return self.cv3(Fn.ConcatFn.apply(None, 0.0, None, self.m(a), self.cv2(x, xsink=sk)), out=out)
        # the last Bottleneck (or the Swin block) and cv2 write their activations straight into the two halves of the
        # concat buffer; a producer that cannot (e.g. an active DropPath) returns its own tensor and ConcatFn copies
        c_ = a.shape[1]
        cat = Fn.concat_buffer(a.shape[0], 2 * c_, a.shape[2], a.shape[3], a)
        if seq:
            for b in blocks[:-1]:
                a = b(a)
            a = blocks[-1](a, out=cat[:, :c_])
        else:
            a = self.m(a, out=cat[:, :c_])
        return self.cv3(Fn.ConcatFn.apply(None, 0.0, None, a, self.cv2(x, xsink=sk, out=cat[:, c_:])), out=out)


class C3Ghost(C3):
    """models/common.py:205-210: C3 whose bottleneck stack is n GhostBottleneck(c_, c_)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


class SPPF(nn.Module):
    """models/common.py:243-258."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    def forward(self, x):
        k = self.m.kernel_size
        c_ = self.cv1.conv.out_channels
        if _INPLACE_CAT >= 1:  # cv1 and the three pools write straight into the concat buffer's slices: no copies
            cat = Fn.concat_buffer(x.shape[0], 4 * c_, x.shape[2], x.shape[3], x)
            sl = [cat[:, i * c_:(i + 1) * c_] for i in range(4)]
        else:
            sl = [None] * 4
        x = self.cv1(x, out=sl[0])
        ys = Fn.maxpool_chain3(x, k, sl[1:])  # inference: the three pools in one launch
        if ys is not None:
            return self.cv2(Fn.ConcatFn.apply(None, 0.0, None, x, *ys))
        s0, s1, s2 = Fn.GradSink(2), Fn.GradSink(2), Fn.GradSink(2)  # each pool input -> next pool + concat
        y1 = Fn.MaxPoolFn.apply(x, k, s0, sl[1:2])
        y2 = Fn.MaxPoolFn.apply(y1, k, s1, sl[2:3])
        return self.cv2(Fn.ConcatFn.apply(None, 0.0, (s0, s1, s2, None), x, y1, y2,
                                          Fn.MaxPoolFn.apply(y2, k, s2, sl[3:4])))


class SPPFCSPC(nn.Module):
    """models/common.py:1257-1276."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=5):
        super().__init__()
        c_ = int(2 * c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(c_, c_, 3, 1)
        self.cv4 = Conv(c_, c_, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
        self.cv5 = Conv(4 * c_, c_, 1, 1)
        self.cv6 = Conv(c_, c_, 3, 1)
        self.cv7 = Conv(2 * c_, c2, 1, 1)

    def forward(self, x):
        k = self.m.kernel_size
        c_ = self.cv1.conv.out_channels
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        if _INPLACE_CAT >= 1:  # every concat input written straight into its slice (cv4 + the pools, cv6 + cv2)
            cat = Fn.concat_buffer(N, 4 * c_, H, W, x)
            sl = [cat[:, i * c_:(i + 1) * c_] for i in range(4)]
            cat2 = Fn.concat_buffer(N, 2 * c_, H, W, x)
            s2l = [cat2[:, :c_], cat2[:, c_:]]
        else:
            sl, s2l = [None] * 4, [None] * 2
        sx = Fn.GradSink(2)  # x -> cv1 and cv2
        x1 = self.cv4(self.cv3(self.cv1(x, xsink=sx)), out=sl[0])
        ys = Fn.maxpool_chain3(x1, k, sl[1:])  # inference: the three pools in one launch
        if ys is not None:
            y1 = self.cv6(self.cv5(Fn.ConcatFn.apply(None, 0.0, None, x1, *ys)), out=s2l[0])
        else:
            s1, s2, s3 = Fn.GradSink(2), Fn.GradSink(2), Fn.GradSink(2)
            x2 = Fn.MaxPoolFn.apply(x1, k, s1, sl[1:2])
            x3 = Fn.MaxPoolFn.apply(x2, k, s2, sl[2:3])
            y1 = self.cv6(self.cv5(Fn.ConcatFn.apply(None, 0.0, (s1, s2, s3, None), x1, x2, x3,
                                                     Fn.MaxPoolFn.apply(x3, k, s3, sl[3:4]))), out=s2l[0])
        y2 = self.cv2(x, xsink=sx, out=s2l[1])
        return self.cv7(Fn.ConcatFn.apply(None, 0.0, None, y1, y2))


class SCConv(nn.Module):
    """Self-calibrated convolution, models/common.py:1279-1316: k4(k3(x) * sigmoid(x + up(k2(x))))."""

    def __init__(self, c1, c2, stride, groups=1, dilation=1, pooling_r=4):
        super().__init__()
        self.k2 = nn.Sequential(nn.AvgPool2d(kernel_size=pooling_r, stride=pooling_r),
                                nn.Conv2d(c1, c1, 3, 1, autopad(3, None), dilation=dilation, groups=groups,
                                          bias=False),
                                nn.BatchNorm2d(c1))
        self.k3 = nn.Sequential(nn.Conv2d(c1, c1, 3, 1, autopad(3, None), dilation=dilation, groups=groups,
                                          bias=False),
                                nn.BatchNorm2d(c1))
        self.k4 = nn.Sequential(nn.Conv2d(c1, c2, 3, stride, autopad(3, None), dilation=dilation, groups=groups,
                                          bias=False),
                                nn.BatchNorm2d(c2))

    def forward(self, x, xsink=None):
        """xsink: the caller's GradSink for x (Model fan-out); this module's three contributions join it"""
        r = self.k2[0].kernel_size
        r = r if isinstance(r, int) else r[0]
        sk = Fn.GradSink(3) if xsink is None else xsink.expect(3)  # x -> avg-pool (k2), k3, the gate
        g = conv_forward(self.k2[1], self.k2[2], None, Fn.AvgPoolFn.apply(x, r, sk))
        u3 = conv_forward(self.k3[0], self.k3[1], None, x, xsink=sk, defer=True)  # BN applied by the gate
        return conv_forward(self.k4[0], self.k4[1], None, Fn.SCGateFn.apply(x, u3, g, sk))


class CoorAttention(nn.Module):
    """Coordinate attention, models/common.py:1158-1207 (YAML token `CA`)."""

    def __init__(self, c1, c2, reduction=32):
        super().__init__()
        self.pool_h = nn.AdaptiveAvgPool2d((None, 1))
        self.pool_w = nn.AdaptiveAvgPool2d((1, None))
        c_ = max(8, c1 // reduction)
        self.conv1 = nn.Conv2d(c1, c_, kernel_size=1, stride=1, padding=0)
        self.bn1 = nn.BatchNorm2d(c_)
        self.act = nn.Hardswish()
        self.conv_w = nn.Conv2d(c_, c2, kernel_size=1, stride=1, padding=0)
        self.conv_h = nn.Conv2d(c_, c2, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        y = conv_forward(self.conv1, self.bn1, self.act, Fn.CAPoolFn.apply(x))   # [N, c_, H+W, 1]
        lh = conv_forward(self.conv_h, None, None, y)                           # logits over all H+W rows
        lw = conv_forward(self.conv_w, None, None, y)
        return Fn.CAApplyFn.apply(x, lh, lw)


CA = CoorAttention  # the north-star YAML's undefined `CA` token binds to CoorAttention


class CABottleneck(nn.Module):
    """models/common.py:1209-1227."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, reduction=32):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.ca = CoorAttention(c2, c2, reduction)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        if not self.add:
            return self.ca(self.cv2(self.cv1(x)))
        sk = Fn.GradSink(2)  # x -> cv1 and the residual
        return Fn.AddFn.apply(x, self.ca(self.cv2(self.cv1(x, xsink=sk))), sk)


class C3CA(C3):
    """models/common.py:1229-1235."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(CABottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))


class Concat(nn.Module):
    """models/common.py:656-664 (channel concat only: the YAML always passes dimension 1)."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def forward(self, x):
        assert self.d == 1
        return Fn.ConcatFn.apply(None, 0.0, None, *x)


def _join(sinks):
    """register one contribution with each given sink; None when there are none"""
    if sinks is None or all(sk is None for sk in sinks):
        return None
    return tuple(sk.expect(1) if sk is not None else None for sk in sinks)


class AdConcat2(nn.Module):
    """BiFPN weighted concat, models/common.py:994-1008."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension
        self.w = nn.Parameter(torch.ones(2, dtype=torch.float32), requires_grad=True)
        self.epsilon = 0.0001

    def forward(self, x, sinks=None):
        """sinks: None or one GradSink-or-None per input (Model fan-out); each joins with one contribution"""
        assert self.d == 1 and len(x) == 2
        return Fn.ConcatFn.apply(self.w, self.epsilon, _join(sinks), *x)


class AdConcat3(AdConcat2):
    """models/common.py:1010-1026."""

    def __init__(self, dimension=1):
        super().__init__(dimension)
        self.w = nn.Parameter(torch.ones(3, dtype=torch.float32), requires_grad=True)

    def forward(self, x, sinks=None):
        assert self.d == 1 and len(x) == 3
        return Fn.ConcatFn.apply(self.w, self.epsilon, _join(sinks), *x)


class SPP(nn.Module):
    """models/common.py:212-227: parallel max-pools (k = 5/9/13, 3/7/11, 3/5/7 in the config-5 YAML)."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])

    def forward(self, x):
        c_, n = self.cv1.conv.out_channels, len(self.m)
        if _INPLACE_CAT >= 1:  # cv1 and every pool write straight into the concat buffer's slices: no copies
            cat = Fn.concat_buffer(x.shape[0], (n + 1) * c_, x.shape[2], x.shape[3], x)
            sl = [cat[:, i * c_:(i + 1) * c_] for i in range(n + 1)]
        else:
            sl = [None] * (n + 1)
        x = self.cv1(x, out=sl[0])
        sk = Fn.GradSink(n + 1)  # x -> every pool and the concat
        ys = [Fn.MaxPoolFn.apply(x, m.kernel_size, sk, sl[i + 1:i + 2]) for i, m in enumerate(self.m)]
        return self.cv2(Fn.ConcatFn.apply(None, 0.0, (sk,) + (None,) * len(ys), x, *ys))


class ChannelAttentionModule(nn.Module):
    """models/common.py:260-285: sigmoid(MLP(avgpool x) + MLP(maxpool x)); both branches go through the
    shared MLP in one [2N]-row pass (1x1 conv kernels), the halves are summed in the sigmoid kernel."""

    def __init__(self, c1, reduction=16):
        super().__init__()
        mid = c1 // reduction
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.shared_MLP = nn.Sequential(nn.Linear(c1, mid), nn.ReLU(), nn.Linear(mid, c1))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x, sink=None):
        l1, l2 = self.shared_MLP[0], self.shared_MLP[2]
        mid, c1 = l1.weight.shape
        z = Fn.GPoolFn.apply(x, sink)
        h = Fn.conv_bn_act(z, l1.weight.view(mid, c1, 1, 1), l1.bias, None, 1, 0, ACT_RELU)
        z2 = Fn.conv_bn_act(h, l2.weight.view(c1, mid, 1, 1), l2.bias, None, 1, 0, ACT_NONE)
        return Fn.HalvesSigmoidFn.apply(z2)


class SpatialAttentionModule(nn.Module):
    """models/common.py:287-300."""

    def __init__(self):
        super().__init__()
        self.conv2d = nn.Conv2d(in_channels=2, out_channels=1, kernel_size=7, stride=1, padding=3)
        self.sigmoid = nn.Sigmoid()

    def forward(self, s2):
        return conv_forward(self.conv2d, None, self.sigmoid, s2)


class CBAM(nn.Module):
    """models/common.py:302-310: out = ca(x) * x;  out = sa(out) * out."""

    def __init__(self, c1, c2):
        super().__init__()
        self.channel_attention = ChannelAttentionModule(c1)
        self.spatial_attention = SpatialAttentionModule()

    def forward(self, x):
        sk = Fn.GradSink(2)  # x -> the pools and the channel scaling
        ca = self.channel_attention(x, sk)
        out1, s2 = Fn.CBAMInFn.apply(x, ca, sk)
        return Fn.PixScaleFn.apply(out1, self.spatial_attention(s2))


class space_to_depth(nn.Module):
    """models/common.py:1451-1458 (SPD: stride-free 2x downsampling into channels)."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def forward(self, x):
        return Fn.SpaceToDepthFn.apply(x)


class SM(space_to_depth):
    """models/common.py:1460-1467: the same cat as space_to_depth under the name the DM YAMLs use."""

    def forward(self, x):
        Fn.even_hw(x.shape[2], x.shape[3], 'SM')
        return Fn.SpaceToDepthFn.apply(x)


class MP(nn.Module):
    """models/common.py:1469-1475: nn.MaxPool2d(k, k).  Only k = 2 has a kernel (dmy_maxpool2_*); `m` is kept for the
    reference's attribute (it has no parameters)."""

    def __init__(self, k=2):
        super().__init__()
        if k != 2:
            raise NotImplementedError(f'MP(k={k}): only the 2 x 2 stride-2 max pool has a gfx950 kernel')
        self.m = nn.MaxPool2d(kernel_size=k, stride=k)

    def forward(self, x, sink=None):
        return Fn.MaxPool2Fn.apply(x, sink)


def _spd_conv(m, x, xsink=None, out=None):
    """a Conv followed by SM, as one spd layer (Fn.conv_bn_act(spd=True))"""
    c, bn = m.conv, getattr(m, 'bn', None)
    assert c.dilation in (1, (1, 1)), 'dilated conv not on the DMA-YOLO path'
    s, pad, a = c.stride[0], _pad_int(c.padding), act_code(m.act)
    return Fn.conv_bn_act(x, c.weight, c.bias, bn, s, pad, a, spec=Fn.spec_for(c, s, pad, a, bn), xsink=xsink, out=out,
                          spd=True)


class DMConv(nn.Module):
    """models/common.py:1538-1547: SM(cv1(x)), cv1 a 3x3 stride-1 Conv -> (N, 4 c2, H / 2, W / 2).  One spd layer: SM
    is folded into cv1's activation pass and into its backward's BN passes."""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = Conv(c1, c2, 3, 1)
        self.sm = SM()

    def forward(self, x, out=None):
        Fn.even_hw(x.shape[2], x.shape[3], 'DMConv')
        return _spd_conv(self.cv1, x, out=out)


class DMMConv(nn.Module):
    """models/common.py:1523-1536: cat(SM(cv2(x)), cv1(MP(x))) -> (N, 5 c2, H / 2, W / 2).  One concat buffer: cv2 (3x3,
    spd) writes the first 4 c2 channels, cv1 over the pooled map the last c2, so the concat copies nothing.  x feeds
    the pool and cv2: their input gradients meet in one GradSink."""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c1, c2, 3, 1)
        self.sm = SM()
        self.mp = MP()

    def forward(self, x):
        N, _, H, W = x.shape
        Fn.even_hw(H, W, 'DMMConv')
        c2 = self.cv2.conv.out_channels
        cat = Fn.concat_buffer(N, 5 * c2, H // 2, W // 2, x)
        sk = Fn.GradSink(2)
        a = _spd_conv(self.cv2, x, xsink=sk, out=cat[:, :4 * c2])
        b = self.cv1(self.mp(x, sk), out=cat[:, 4 * c2:])
        return Fn.ConcatFn.apply(None, 0.0, None, a, b)


class DMMConv2(nn.Module):
    """models/common.py:1508-1521: cat(SM(x), cv1(MP(x))) -> (N, 4 c1 + c2, H / 2, W / 2).  Fn.SpdSplitFn reads x once
    and writes SM(x) into the first 4 c1 channels of the concat buffer and the pooled map; cv1 writes the last c2."""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.sm = SM()
        self.mp = MP()

    def forward(self, x):
        N, c1, H, W = x.shape
        Fn.even_hw(H, W, 'DMMConv2')
        c2 = self.cv1.conv.out_channels
        cat = Fn.concat_buffer(N, 4 * c1 + c2, H // 2, W // 2, x)
        a, p = Fn.SpdSplitFn.apply(x, [cat[:, :4 * c1]])
        b = self.cv1(p, out=cat[:, 4 * c1:])
        return Fn.ConcatFn.apply(None, 0.0, None, a, b)


class _AddConv(nn.Sequential):
    """add_conv's stage, models/common.py:1063-1081: conv (no bias) -> batch_norm -> LeakyReLU(0.1), with the
    reference's child names.  Model.fuse() leaves its BN alone, as the reference does (it fuses Conv / DWConv only)."""

    def forward(self, x, xsink=None, out=None):
        return conv_forward(self.conv, self.batch_norm, self.leaky, x, xsink=xsink, out=out)


def add_conv(in_ch, out_ch, ksize=1, stride=1):
    """models/common.py:1063-1081."""
    stage = _AddConv()
    stage.add_module('conv', nn.Conv2d(in_ch, out_ch, ksize, stride, (ksize - 1) // 2, bias=False))
    stage.add_module('batch_norm', nn.BatchNorm2d(out_ch))
    stage.add_module('leaky', nn.LeakyReLU(0.1))
    return stage


def _fan(sinks, i, k):
    """input i's GradSink with k more contributions registered: the caller's, or a fresh one for k > 1"""
    sk = sinks[i] if sinks is not None else None
    if sk is not None:
        return sk.expect(k)
    return Fn.GradSink(k) if k > 1 else None


class AdaptConcat(nn.Module):
    """Concat with per-pixel learned weights, models/common.py:953-992: each input's add_conv gives 16 level-map
    channels, weight_levels (a 1x1 conv with bias) turns them into one logit per input, and the inputs are scaled by the
    softmax of the logits before the concat.  The add_conv stages write their maps side by side into one buffer and one
    kernel does weight_levels, the softmax, the scaling and the concat (Fn.AdaptGateFn).  A level-2 module keeps the
    reference's weight_map2 (dim3 = 1), which no forward uses."""

    def __init__(self, level, dimension, dim1, dim2, dim3=1, rfb=False):
        super().__init__()
        self.level, self.d, self.dims = level, dimension, [dim1, dim2, dim3]
        compress_c = 8 if rfb else 16
        self.weight_map0 = add_conv(self.dims[0], compress_c, 1, 1)
        self.weight_map1 = add_conv(self.dims[1], compress_c, 1, 1)
        self.weight_map2 = add_conv(self.dims[2], compress_c, 1, 1)
        self.weight_levels = nn.Conv2d(compress_c * level, level, kernel_size=1, stride=1, padding=0)

    def forward(self, x, sinks=None):
        """sinks: None or one GradSink-or-None per input (Model fan-out); each input has two consumers here, its
        add_conv and the gate, which accumulate into one buffer"""
        L = self.level
        assert self.d == 1 and L in (2, 3) and len(x) == L
        cc = self.weight_map0.conv.out_channels
        N, _, H, W = x[0].shape
        sks = [_fan(sinks, i, 2) for i in range(L)]
        wm = Fn.concat_buffer(N, cc * L, H, W, x[0])
        maps = [getattr(self, f'weight_map{i}')(x[i], xsink=sks[i], out=wm[:, cc * i:cc * (i + 1)]) for i in range(L)]
        wm = Fn.ConcatFn.apply(None, 0.0, None, *maps)
        return Fn.AdaptGateFn.apply(self.weight_levels.weight, self.weight_levels.bias, tuple(sks), wm, *x)


class Adapt_Add2(nn.Module):
    """models/common.py:1028-1044: silu(w0' x0 + w1' x1), w' = w / (sum w + 1e-4)."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(2, dtype=torch.float32), requires_grad=True)
        self.epsilon = 0.0001
        self.silu = nn.SiLU()

    def forward(self, x, sinks=None):
        assert len(x) == 2
        return Fn.AdaptAddFn.apply(self.w, self.epsilon, _join(sinks), *x)


class Adapt_Add3(nn.Module):
    """models/common.py:1046-1061: silu(w0' conv(x0) + w1' conv(x1) + w2' x2), one 1x1 conv (bias, no BN, no activation)
    applied to both x0 and x1."""

    def __init__(self, d1, d2, d3):
        super().__init__()
        self.w = nn.Parameter(torch.ones(3, dtype=torch.float32), requires_grad=True)
        self.epsilon = 0.0001
        self.conv = nn.Conv2d(d1, d3, kernel_size=1, stride=1, padding=0)
        self.silu = nn.SiLU()

    def forward(self, x, sinks=None):
        assert len(x) == 3
        a = conv_forward(self.conv, None, None, x[0], xsink=_fan(sinks, 0, 1))
        b = conv_forward(self.conv, None, None, x[1], xsink=_fan(sinks, 1, 1))
        return Fn.AdaptAddFn.apply(self.w, self.epsilon, (None, None, _fan(sinks, 2, 1)), a, b, x[2])


class AdaptADD(nn.Module):
    """models/common.py:912-951 does not construct in the reference itself (its __init__ lacks an argument that
    parse_model passes); not provided."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('AdaptADD (adaptadd.yaml) does not build in the reference and is not provided; '
                                  'use AdaptConcat or Adapt_Add2 / Adapt_Add3')


class Upsample(nn.Upsample):
    """nn.Upsample(None, 2, 'nearest') as used by the YAML heads; nearest only.  out: a concat_buffer slice to write
    the result into (Model's concat plan)."""

    def forward(self, x, out=None):
        assert self.mode == 'nearest'
        H, W = x.shape[2:]
        if self.size is not None:
            OH, OW = (self.size, self.size) if isinstance(self.size, int) else self.size
        else:
            sf = self.scale_factor if isinstance(self.scale_factor, (tuple, list)) else (self.scale_factor,) * 2
            OH, OW = int(math.floor(H * sf[0])), int(math.floor(W * sf[1]))
        return Fn.ResizeFn.apply(x, OH, OW, [out] if out is not None else None)


# ------------------------------------------------------------------ Swin (C3STR) — layers in swin.py
from .swin import SwinTransformerBlock, SwinTransformerLayer, WindowAttention, Mlp, DropPath  # noqa: E402


class C3STR(C3):
    """models/common.py:191-196: C3 whose bottleneck stack is a 3-layer Swin block (heads = c_ // 32)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = SwinTransformerBlock(c_, c_, c_ // 32, n)


# ------------------------------------------------------------------ HorNet: GnConv / HorBlock / C3HB (csrc/hor.hip)

class LayerNorm(nn.Module):
    """models/common.py:1402-1427.  Activations here are NHWC whatever the reference's layout at that point, so both
    data formats are Fn.LayerNormFn over the channels (the channels_first formula is the same biased-variance norm)."""

    def __init__(self, normalized_shape, eps=1e-6, data_format='channels_last'):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        if self.data_format not in ['channels_last', 'channels_first']:
            raise NotImplementedError
        self.normalized_shape = (normalized_shape,)

    def forward(self, x, sink=None):
        return Fn.LayerNormFn.apply(x, self.weight, self.bias, self.eps, sink)


class GnConv(nn.Module):
    """Recursive gated convolution, models/common.py:1318-1359.  proj_in writes one 2 * c1-channel buffer; the biased
    depthwise 7x7 reads its abc slice in place (pixel stride 2 * c1) and the gates read pwa and the dw_list slices
    through Fn.SplitFn views, so torch.split copies nothing; in the backward every gate writes its slice of d(dw_abc) /
    d(fused_x) directly (Fn.SliceSink).  `scale` is applied by the gate kernel."""

    def __init__(self, c1, c2, ksize=1, stride=1, order=5, gflayer=None, h=14, w=8, s=1.0):
        super().__init__()
        if gflayer is not None:
            raise NotImplementedError('GnConv: gflayer (the global-filter depthwise layer) has no gfx950 kernel')
        self.order = order
        self.dims = [c1 // 2 ** i for i in range(order)]
        self.dims.reverse()
        self.proj_in = nn.Conv2d(c1, 2 * c1, 1)
        sd = sum(self.dims)
        self.dwconv = nn.Conv2d(sd, sd, kernel_size=7, padding=3, bias=True, groups=sd)  # get_dwconv(sd, 7, True)
        self.proj_out = Conv(c1, c2, ksize, stride)
        self.pws = nn.ModuleList([nn.Conv2d(self.dims[i], self.dims[i + 1], 1) for i in range(order - 1)])
        self.scale = s

    def _check(self, x):
        """every gate operand is a whole number of 16-byte vectors at a vector offset of its buffer"""
        c1 = self.proj_in.in_channels
        vw = Fn.VW.get(x.dtype)
        if vw is None or c1 % 2 ** (self.order - 1) or any(d % vw for d in self.dims):
            raise NotImplementedError(f'GnConv: c1={c1} gives the gate widths {self.dims}, which must be multiples of '
                                      f'{vw} channels for {x.dtype} (c1 >= {16 * (vw or 0)} at order 5)')

    def forward(self, x, mask=None, dummy=False, res=None, rsink=None, out=None):
        """res / rsink / out: proj_out's residual, its GradSink and a concat_buffer slice, as Conv.forward"""
        self._check(x)
        dims, sd = self.dims, sum(self.dims)
        fused = conv_forward(self.proj_in, None, None, x)
        grad = torch.is_grad_enabled()
        sf = Fn.SliceSink(2, fused) if grad else None  # d(fused_x): pwa's slice from gate 0, abc's from the dwconv
        pwa = Fn.SplitFn.apply(fused, 0, dims[0], sf)
        abc = Fn.SplitFn.apply(fused, dims[0], sd, sf)
        dw = conv_forward(self.dwconv, None, None, abc, xsink=sf.part(dims[0], sd) if grad else None)
        sw = Fn.SliceSink(self.order, dw) if grad else None  # d(dw_abc): one slice per gate
        a, c0 = pwa, 0
        for i, d in enumerate(dims):
            if i:
                a = conv_forward(self.pws[i - 1], None, None, a)
            a = Fn.GateMulFn.apply(a, Fn.SplitFn.apply(dw, c0, d, sw), self.scale,
                                   sf.part(0, d) if grad and i == 0 else None, sw.part(c0, d) if grad else None)
            c0 += d
        return self.proj_out(a, res=res, rsink=rsink, out=out)


class HorBlock(nn.Module):
    """models/common.py:1364-1400: x + gamma1 * gnconv(norm1(x)), then x + gamma2 * pwconv2(gelu(pwconv1(norm2(x)))).
    As in the reference the block builds GnConv(dim, dim) whatever `gnconv` names."""

    dmy_out = True  # forward(x, out=view) writes its result into a concat_buffer slice when it can (C3.forward)

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6, gnconv=GnConv):
        super().__init__()
        if drop_path > 0.:
            raise NotImplementedError('HorBlock: drop_path > 0 has no gfx950 path (no YAML reaches it)')
        self.norm1 = LayerNorm(dim, eps=1e-6, data_format='channels_first')
        self.gnconv = GnConv(dim, dim)
        self.norm2 = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma1 = nn.Parameter(layer_scale_init_value * torch.ones(dim),
                                   requires_grad=True) if layer_scale_init_value > 0 else None
        self.gamma2 = nn.Parameter(layer_scale_init_value * torch.ones((dim)),
                                   requires_grad=True) if layer_scale_init_value > 0 else None
        self.drop_path = nn.Identity()

    def forward(self, x, out=None):
        """out: a concat_buffer slice the second residual sum is written into (C3HB's last block)"""
        c = x.shape[1]
        self.gnconv._check(x)
        s1, s2 = Fn.GradSink(2), Fn.GradSink(2)  # x -> norm1 + residual; x2 -> norm2 + residual
        u = self.norm1(x, s1)
        if self.gamma1 is None:
            x = self.gnconv(u, res=x, rsink=s1)
        else:
            x = Fn.LayerScaleAddFn.apply(x, self.gnconv(u), self.gamma1, s1)
        u2 = self.norm2(x, s2)
        h = Fn.conv_bn_act(u2, self.pwconv1.weight.view(4 * c, c, 1, 1), self.pwconv1.bias, None, 1, 0, Fn.ACT_GELU)
        w2, b2 = self.pwconv2.weight.view(c, 4 * c, 1, 1), self.pwconv2.bias
        if self.gamma2 is None:
            return Fn.conv_bn_act(h, w2, b2, None, 1, 0, Fn.ACT_NONE, res=x, rsink=s2, out=out)
        return Fn.LayerScaleAddFn.apply(x, Fn.conv_bn_act(h, w2, b2, None, 1, 0, Fn.ACT_NONE), self.gamma2, s2,
                                        [out] if out is not None else None)


class _OutStack(nn.Sequential):
    """C3HB.m / CSPCM.m: blocks whose forward takes out= in sequence, the last one writing into C3's concat buffer"""
    dmy_out = True

    def forward(self, x, out=None):
        blocks = list(self)
        for b in blocks[:-1]:
            x = b(x)
        return blocks[-1](x, out=out) if blocks else x


class C3HB(C3):
    """models/common.py:1429-1439: C3 whose bottleneck stack is n HorBlock(c_)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = _OutStack(*(HorBlock(c_) for _ in range(n)))


# ------------------------------------------------------------------ ConvMixer: ConvMix / CSPCM (csrc/convmix.hip)

class _ActBNStage(nn.Sequential):
    """conv (with bias) -> GELU -> BatchNorm2d, the stage both halves of ConvMix are made of (models/cspcm.py:28-37),
    with the reference's child indices 0 / 1 / 2.  The activation comes BEFORE the BN, so the stage runs on
    Fn.conv_act_bn.  Model.fuse() leaves it alone, as the reference does (it fuses Conv / DWConv only)."""

    def forward(self, x, res=None, xsink=None, rsink=None, out=None):
        conv, act, bn = self[0], self[1], self[2]
        k, s = conv.kernel_size[0], conv.stride[0]
        pad = k // 2 if conv.padding == 'same' else _pad_int(conv.padding)
        a = act_code(act)
        return Fn.conv_act_bn(x, conv.weight, conv.bias, bn, s, pad, a, res=res, spec=Fn.spec_for(conv, s, pad, a, bn),
                              xsink=xsink, rsink=rsink, out=out)


class ConvMix(nn.Module):
    """ConvMixer block, models/cspcm.py:25-41: x + BN(GELU(dw9x9(x))), then BN(GELU(conv1x1(.))); both convs biased.
    The residual add rides on the first stage's act-BN pass (inference: on the depthwise launch itself).  As in the
    reference, dim1 is not used."""

    dmy_out = True  # forward(x, out=view) writes its result into a concat_buffer slice (C3.forward)

    def __init__(self, dim, dim1, kernel_size=9):
        super().__init__()
        if kernel_size != 9:
            raise NotImplementedError(f'ConvMix: kernel_size={kernel_size} has no gfx950 kernel (only the depthwise 9x9 of '
                                      'models/cspcm.py:26)')
        if dim % 4:
            raise NotImplementedError(f'ConvMix: dim={dim} is not a whole number of 16-byte vectors (multiples of 4 '
                                      'channels for float32, 8 for bfloat16)')
        self.Resnet = _ActBNStage(nn.Conv2d(dim, dim, kernel_size=kernel_size, groups=dim, padding='same'), nn.GELU(),
                                  nn.BatchNorm2d(dim))
        self.Conv_1x1 = _ActBNStage(nn.Conv2d(dim, dim, kernel_size=1), nn.GELU(), nn.BatchNorm2d(dim))

    def forward(self, x, out=None):
        vw = Fn.VW.get(x.dtype)
        if vw is None or x.shape[1] % vw:
            raise NotImplementedError(f'ConvMix: {x.shape[1]} channels are not a whole number of 16-byte vectors of '
                                      f'{x.dtype} (multiples of {vw})')
        sk = Fn.GradSink(2)  # x -> the depthwise conv and the residual
        x = self.Resnet(x, res=x, xsink=sk, rsink=sk)
        return self.Conv_1x1(x, out=out)


class CSPCM(C3):
    """models/cspcm.py:43-54: C3's cv1 | cv2 -> concat -> cv3 around n ConvMix(c_, c_)."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__(c1, c2, n, True, 1, e)
        c_ = int(c2 * e)
        self.m = _OutStack(*(ConvMix(c_, c_) for _ in range(n)))


# ------------------------------------------------------------------ C3TR (config 5: global MHSA over P5 tokens)

class TransformerLayer(nn.Module):
    """models/common.py:312-336: x + Dropout(MHA(q(LN1 x), k(LN1 x), v(LN1 x))); x + Dropout(fc2(Dropout(
    ReLU(fc1(LN2 x))))).  `ma` is the real nn.MultiheadAttention (state_dict keys ma.in_proj_weight /
    in_proj_bias / out_proj.*; train.py's optimizer grouping skips in_proj_*); its
    projections run on the implicit-GEMM kernels and the attention core on csrc/mha.hip.  Tokens are
    the pixels of the NHWC activation, so the reference's [HW, b, c] sequence-first transposes are free."""

    def __init__(self, c, num_heads):
        super().__init__()
        self.ln1 = nn.LayerNorm(c)
        self.q = nn.Linear(c, c, bias=False)
        self.k = nn.Linear(c, c, bias=False)
        self.v = nn.Linear(c, c, bias=False)
        self.ma = nn.MultiheadAttention(embed_dim=c, num_heads=num_heads)
        self.ln2 = nn.LayerNorm(c)
        self.fc1 = nn.Linear(c, 4 * c, bias=False)
        self.fc2 = nn.Linear(4 * c, c, bias=False)
        self.dropout = nn.Dropout(0.1)
        self.act = nn.ReLU(True)

    @staticmethod
    def _lin(x, w, b=None, act=ACT_NONE, **kw):
        return Fn.conv_bn_act(x, w.view(w.shape[0], w.shape[1], 1, 1), b, None, 1, 0, act, **kw)

    def forward(self, x):
        c = x.shape[1]
        ma = self.ma
        drop = self.training and self.dropout.p > 0
        p = self.dropout.p
        s1, su, s2 = Fn.GradSink(2), Fn.GradSink(3), Fn.GradSink(2)  # x -> ln1 + residual; u -> q/k/v; x2 -> ln2 + residual
        u = Fn.LayerNormFn.apply(x, self.ln1.weight, self.ln1.bias, self.ln1.eps, s1)
        W, bi = ma.in_proj_weight, ma.in_proj_bias
        q = self._lin(self._lin(u, self.q.weight, xsink=su), W[:c], bi[:c])
        k = self._lin(self._lin(u, self.k.weight, xsink=su), W[c:2 * c], bi[c:2 * c])
        v = self._lin(self._lin(u, self.v.weight, xsink=su), W[2 * c:], bi[2 * c:])
        o = Fn.MHAFn.apply(q, k, v, ma.num_heads)
        if drop:
            x = Fn.AddFn.apply(x, Fn.DropoutFn.apply(self._lin(o, ma.out_proj.weight, ma.out_proj.bias), p), s1)
        else:
            x = self._lin(o, ma.out_proj.weight, ma.out_proj.bias, res=x, rsink=s1)
        u2 = Fn.LayerNormFn.apply(x, self.ln2.weight, self.ln2.bias, self.ln2.eps, s2)
        h = self._lin(u2, self.fc1.weight, act=ACT_RELU)
        if drop:
            return Fn.AddFn.apply(x, Fn.DropoutFn.apply(self._lin(Fn.DropoutFn.apply(h, p), self.fc2.weight), p), s2)
        return self._lin(h, self.fc2.weight, res=x, rsink=s2)


class TransformerBlock(nn.Module):
    """models/common.py:338-355: (optional Conv) -> p + linear(p) (learned position term, residual fused
    into the GEMM epilogue) -> n TransformerLayers; tokens stay in the NHWC activation."""

    def __init__(self, c1, c2, num_heads, num_layers):
        super().__init__()
        self.conv = None
        if c1 != c2:
            self.conv = Conv(c1, c2)
        self.linear = nn.Linear(c2, c2)
        self.tr = nn.Sequential(*(TransformerLayer(c2, num_heads) for _ in range(num_layers)))
        self.c2 = c2

    def forward(self, x):
        if self.conv is not None:
            x = self.conv(x)
        sk = Fn.GradSink(2)  # p -> linear + residual
        w = self.linear.weight
        p = Fn.conv_bn_act(x, w.view(self.c2, self.c2, 1, 1), self.linear.bias, None, 1, 0, ACT_NONE, res=x,
                           xsink=sk, rsink=sk)
        return self.tr(p)


class C3TR(C3):
    """models/common.py:184-189: C3 whose bottleneck stack is TransformerBlock(c_, c_, 4 heads, n)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = TransformerBlock(c_, c_, 4, n)


# ------------------------------------------------------------------ AutoShape (models/common.py:701-891)

# one image of dmy_letterbox_batch (csrc/autoshape.hip LetterboxDesc; sizeof = dmy_letterbox_desc_bytes)
LETTERBOX_DESC = np.dtype([('src', '<u8'), ('xt', '<u8'), ('yt', '<u8'), ('H0', '<i4'), ('W0', '<i4'), ('h', '<i4'),
                           ('w', '<i4'), ('top', '<i4'), ('left', '<i4'), ('swap', '<i4'), ('pad', '<i4')])


def autoshape_geometry(shapes, size, stride):
    """Host geometry of AutoShape.forward (models/common.py:769-775, 790) for images of `shapes` = [(H0, W0), ...]:
    (shape1, [(h, w, top, left, gain, (pad_x, pad_y)) per image]).  shape1 is the batch's inference shape; (h, w) the
    unpadded size and (top, left) the border letterbox(im, new_shape=shape1, auto=False) gives the image
    (utils/augmentations.py:92-123); gain and pad are what scale_coords(shape1, ., (H0, W0)) computes, in double."""
    shape1 = [[y * (size / max(s)) for y in s] for s in shapes]
    shape1 = [make_divisible(x, stride) for x in np.stack(shape1, 0).max(0)]
    geo = []
    for H0, W0 in shapes:
        r = min(shape1[0] / H0, shape1[1] / W0)
        w, h = int(round(W0 * r)), int(round(H0 * r))
        dw, dh = (shape1[1] - w) / 2, (shape1[0] - h) / 2
        top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
        gain = min(shape1[0] / H0, shape1[1] / W0)
        geo.append((h, w, top, left, gain, ((shape1[1] - W0 * gain) / 2, (shape1[0] - H0 * gain) / 2)))
    return shape1, geo


@functools.lru_cache(maxsize=64)
def _resize_table(dst, src):
    from ..augment import _resize_table as table
    return table(dst, src)


def letterbox_batch(imgs, shape1, geo, dtype, s2d, device, swap=False, stage=None):
    """The stem input of a batch of decoded images (uint8 HWC, 3 channels, C-contiguous numpy arrays), letterboxed to
    `shape1` with `geo` (autoshape_geometry) by ONE dmy_letterbox_batch launch: `dtype` in NHWC storage, space-to-depth
    (`_dmy_s2d`, as Fn.image_s2d) or channel-padded (`_dmy_cpad`, as Model.to_input's ToNHWC).  The images, their
    resize tables and the descriptors travel in one non-blocking copy from a pinned staging buffer (`stage`, a
    one-element list that keeps it between calls)."""
    assert call('dmy_letterbox_desc_bytes') == LETTERBOX_DESC.itemsize, 'LetterboxDesc layout mismatch'
    n, (OH, OW) = len(imgs), shape1
    parts, total = [], 0  # (offset, uint8 view) of everything the kernel reads

    def put(a):
        nonlocal total
        off = -(-total // 16) * 16
        parts.append((off, a.reshape(-1).view(np.uint8)))
        total = off + a.nbytes
        return off

    d = np.zeros(n, dtype=LETTERBOX_DESC)
    for k, (im, (h, w, top, left, _, _)) in enumerate(zip(imgs, geo)):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise TypeError(f'image {k}: the letterbox kernel takes uint8 HWC images of 3 channels, got {im.dtype} '
                            f'{im.shape}')
        H0, W0 = im.shape[:2]
        d[k]['src'], d[k]['xt'], d[k]['yt'] = put(np.ascontiguousarray(im)), put(_resize_table(w, W0)), \
            put(_resize_table(h, H0))
        d[k]['H0'], d[k]['W0'], d[k]['h'], d[k]['w'], d[k]['top'], d[k]['left'] = H0, W0, h, w, top, left
        d[k]['swap'] = int(bool(swap))
    doff = -(-total // 16) * 16
    total = doff + d.nbytes
    stage = [None] if stage is None else stage
    if stage[0] is None or stage[0][0].numel() < total:
        stage[0] = (torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
    pinned, copied = stage[0]
    copied.synchronize()  # the previous batch's copy has left the buffer
    dev = torch.empty(total, dtype=torch.uint8, device=device)
    base, host = dev.data_ptr(), pinned.numpy()
    for f in ('src', 'xt', 'yt'):
        d[f] += base
    for off, a in parts:
        host[off:off + a.size] = a
    host[doff:total] = d.view(np.uint8)
    dev.copy_(pinned[:total], non_blocking=True)
    copied.record()
    if s2d:
        Cs = Fn.vec_pad(12, dtype)
        buf = torch.empty((n, Cs, OH // 2, OW // 2), dtype=dtype, device=device, memory_format=Fn.CL)
    else:
        Cs = Fn.vec_pad(3, dtype)
        buf = torch.empty((n, Cs, OH, OW), dtype=dtype, device=device, memory_format=Fn.CL)
    call('dmy_letterbox_batch', Fn.DT[dtype], ctypes.c_void_p(base + doff), ctypes.c_void_p(pinned.data_ptr() + doff),
         n, ptr(buf), OH, OW, int(bool(s2d)), Cs, 1.0 / 255.0, stream())
    if s2d:
        buf._dmy_s2d = 3
        return buf
    y = buf[:, :3] if Cs != 3 else buf
    y._dmy_cpad = Cs
    return y


def scale_boxes(out, counts, geo, shapes):
    """scale_coords (utils/general.py:605-617) of every image's rows of the padded NMS buffer `out`
    (nimg, max_det, 6), in place, plus the Detections conversions (models/common.py:805-808), by ONE dmy_scale_boxes
    launch: -> (xywh, xyxyn, xywhn), buffers of out's shape of which the first counts[b] rows of image b are written"""
    nimg, max_det = out.shape[:2]
    g = np.empty(6 * nimg, dtype=np.float32)  # [gain, pad_x, pad_y, w0, h0] per image, then the int32 keep counts
    g[:5 * nimg] = [v for (_, _, _, _, gain, pad), (h0, w0) in zip(geo, shapes) for v in (gain, pad[0], pad[1], w0, h0)]
    g[5 * nimg:].view(np.int32)[:] = counts
    gd = torch.from_numpy(g).to(out.device)
    extra = torch.empty((3,) + tuple(out.shape), dtype=torch.float32, device=out.device)
    call('dmy_scale_boxes', ptr(out), ctypes.c_void_p(gd.data_ptr() + 20 * nimg), ptr(gd), ptr(extra[0]),
         ptr(extra[1]), ptr(extra[2]), nimg, max_det, stream())
    return extra[0], extra[1], extra[2]


class AutoShape(nn.Module):
    """models/common.py:701-793: input-robust wrapper -- raw images in, Detections out.  The host computes geometry
    and resize tables only; letterbox, / 255, layout and cast are one dmy_letterbox_batch launch, the mapping of the
    boxes back to each image one dmy_scale_boxes launch (csrc/autoshape.hip).

    Accepted inputs: a numpy uint8 array (HWC; CHW when shape[0] < 5; 2-D grey; extra channels dropped), a PIL image,
    a str / Path file name (decoded through PIL with the EXIF orientation applied), or a list of them; a torch.Tensor
    goes straight to the model.  An http(s) URI raises NotImplementedError (the project has no network client), a
    non-uint8 array TypeError."""
    conf = 0.25  # NMS confidence threshold
    iou = 0.45  # NMS IoU threshold
    classes = None  # (optional list) filter by class
    multi_label = False  # NMS multiple labels per box
    max_det = 1000  # maximum number of detections per image

    def __init__(self, model):
        super().__init__()
        self.model = model.eval()
        self._stage = [None]  # pinned staging buffer of letterbox_batch, kept between calls

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_stage'] = [None]  # a copy or a pickle of the wrapper gets a staging buffer of its own
        return state

    def autoshape(self):
        _LOG.info('AutoShape already enabled, skipping... ')
        return self

    def _prepare(self, imgs):
        """models/common.py:756-773: -> (n, images as contiguous uint8 HWC RGB arrays, file names)"""
        from PIL import Image, ImageOps
        n, imgs = (len(imgs), list(imgs)) if isinstance(imgs, (list, tuple)) else (1, [imgs])
        files = []
        for i, im in enumerate(imgs):
            f = f'image{i}'
            if isinstance(im, (str, Path)):
                if str(im).startswith('http'):
                    raise NotImplementedError(f'{im}: fetching an image over the network is not supported, pass a '
                                              'local file or a decoded image')
                from ..data import _read_bgr
                im, f = _read_bgr(str(im), rgb=True), im
            elif isinstance(im, Image.Image):
                im, f = np.asarray(ImageOps.exif_transpose(im)), getattr(im, 'filename', f) or f
            elif not isinstance(im, np.ndarray):
                raise TypeError(f'image {i}: expected a numpy array, a PIL image or a file name, got {type(im).__name__}')
            files.append(Path(f).with_suffix('.jpg').name)
            if im.shape[0] < 5:  # image in CHW
                im = im.transpose((1, 2, 0))
            im = im[..., :3] if im.ndim == 3 else np.tile(im[..., None], 3)
            imgs[i] = np.ascontiguousarray(im)
        return n, imgs, files

    @torch.no_grad()
    def forward(self, imgs, size=640, augment=False, profile=False):
        t = [time_sync()]
        p = next(self.model.parameters())
        if isinstance(imgs, torch.Tensor):
            return self.model(imgs.to(p.device), augment, profile)
        if p.device.type != 'cuda':
            raise RuntimeError('AutoShape runs on the GPU: move the model there first (there is no CPU path)')
        n, imgs, files = self._prepare(imgs)
        m = self.model
        shapes = [im.shape[:2] for im in imgs]
        shape1, geo = autoshape_geometry(shapes, size, int(getattr(self, 'stride', m.stride).max()))
        if augment:
            # the augmented forward resamples the NCHW image itself: hand it the letterboxed batch as fp32 planes
            # (level * 1/255, the value its own uint8 path forms per tap)
            x = letterbox_batch(imgs, shape1, geo, torch.float32, False, p.device, stage=self._stage).contiguous()
        else:
            s2d = m._s2d_stem(torch.empty((n, 3, *shape1), device='meta'))
            x = letterbox_batch(imgs, shape1, geo, m.act_dtype, s2d, p.device, stage=self._stage)
        t.append(time_sync())
        y = m(x, augment, profile)[0]
        t.append(time_sync())
        out, pred = nms_padded(y, self.conf, iou_thres=self.iou, classes=self.classes, multi_label=self.multi_label,
                               max_det=self.max_det)
        xywh, xyxyn, xywhn = scale_boxes(out, [q.shape[0] for q in pred], geo, shapes)
        extra = [[b[i, :q.shape[0]] for i, q in enumerate(pred)] for b in (xywh, xyxyn, xywhn)]
        t.append(time_sync())
        return Detections(imgs, pred, files, t, getattr(self, 'names', m.names), torch.Size((n, 3, *shape1)), *extra)


class Detections:
    """models/common.py:795-891: the results of one AutoShape call.  `pred` / `xyxy` are the per-image (k, 6) rows
    (xyxy pixels of the original image, conf, cls), `xywh` the centre form, `xyxyn` / `xywhn` those divided by the
    image's (w, h, w, h); `t` is ms per image of pre-process / inference / NMS.  AutoShape hands over the converted
    rows its box kernel wrote; built by hand (xywh=None) they are computed with the reference's torch expressions."""

    def __init__(self, imgs, pred, files, times=None, names=None, shape=None, xywh=None, xyxyn=None, xywhn=None):
        self.imgs = imgs  # list of images as numpy arrays
        self.pred = pred  # list of tensors pred[0] = (xyxy, conf, cls)
        self.names = names
        self.files = files
        self.xyxy = pred
        if xywh is None:
            gn = [torch.tensor([*(im.shape[i] for i in [1, 0, 1, 0]), 1, 1], device=q.device) for im, q in zip(imgs, pred)]
            xywh = [xyxy2xywh(x) for x in pred]
            xyxyn = [x / g for x, g in zip(pred, gn)]
            xywhn = [x / g for x, g in zip(xywh, gn)]
        self.xywh, self.xyxyn, self.xywhn = xywh, xyxyn, xywhn
        self.n = len(self.pred)
        self.t = tuple((times[i + 1] - times[i]) * 1000 / self.n for i in range(3)) if times is not None else None
        self.s = shape  # inference BCHW shape

    def _summary(self):
        """one line per image, as display(pprint=True) logs it (models/common.py:815-837)"""
        lines = []
        for i, (im, pred) in enumerate(zip(self.imgs, self.pred)):
            s = f'image {i + 1}/{len(self.pred)}: {im.shape[0]}x{im.shape[1]} '
            if pred.shape[0]:
                for c in pred[:, -1].unique():
                    k = int((pred[:, -1] == c).sum())
                    s += f"{k} {self.names[int(c)]}{'s' * (k > 1)}, "
            else:
                s += '(no detections)'
            lines.append(s.rstrip(', '))
        return lines

    def __str__(self):
        s = '\n'.join(self._summary())
        if self.t is not None:
            s += f'\nSpeed: %.1fms pre-process, %.1fms inference, %.1fms NMS per image at shape {tuple(self.s)}' % self.t
        return s

    def print(self):
        for line in str(self).split('\n'):
            _LOG.info(line)

    def _no_plot(self, *args, **kwargs):
        raise NotImplementedError('show / save / crop / render need the plotting code (Annotator, save_one_box), '
                                  'which this project does not have')

    show = save = crop = render = _no_plot

    def pandas(self):
        """models/common.py:872-880: a copy whose xyxy / xyxyn / xywh / xywhn are lists of pandas DataFrames"""
        import pandas as pd
        new = copy(self)
        ca = 'xmin', 'ymin', 'xmax', 'ymax', 'confidence', 'class', 'name'
        cb = 'xcenter', 'ycenter', 'width', 'height', 'confidence', 'class', 'name'
        for k, c in zip(['xyxy', 'xyxyn', 'xywh', 'xywhn'], [ca, ca, cb, cb]):
            a = [[x[:5] + [int(x[5]), self.names[int(x[5])]] for x in x.tolist()] for x in getattr(self, k)]
            setattr(new, k, [pd.DataFrame(x, columns=c) for x in a])
        return new

    def tolist(self):
        """One Detections per image, its imgs / pred / xyxy / xyxyn / xywh / xywhn popped out of their lists as the
        reference does (models/common.py:882-888).  Deviation: the reference builds each with
        Detections([img], [pred], self.names, self.s), which puts `names` in the `files` position and the shape in the
        `times` position; here every field is the image's own (files = [its file], names, t and s kept)."""
        res = []
        for i in range(self.n):
            d = copy(self)
            for k in ('imgs', 'pred', 'xyxy', 'xyxyn', 'xywh', 'xywhn'):
                setattr(d, k, getattr(self, k)[i])
            d.files, d.n = [self.files[i]], 1
            res.append(d)
        return res

    def __len__(self):
        return self.n
