"""The e4m3 forward of the eligible convs (csrc/conv.hip dmy_conv_fwd_fp8, dmy_fp8_quant; csrc/bn.hip
dmy_bn_act_fwd_f8): operand quantisation, the per-spec weight cache and delayed activation scaling.  conv.py calls
into this module; the two model-level entry points set_fp8 / f8_saturation walk conv.py's spec registry and live
there."""
import os

import torch

from .._lib import call, ptr, stream
from ._base import f32


def fp8_eligible(C, K, dtype, rows):
    """layers the e4m3 forward kernel takes (dmy_conv_fwd_fp8): bf16 activations, C % 128 == 0 (one 128-wide
    K step per tap), K % 8 == 0, and byte offsets of the quantised input below the buffer-descriptor range"""
    return dtype == torch.bfloat16 and C % 128 == 0 and K % 8 == 0 and K >= 32 and rows * C < 0xFFFFFFF0


_F8_WS = [0]


def _f8_ws():
    _F8_WS[0] = call('dmy_fp8_quant_ws_elems')
    return _F8_WS[0]


# delayed (previous-step) activation scaling for the fp8 convs: the producing layer emits the e4m3 copy of its
# output in its BN-act pass (dmy_bn_act_fwd_f8) instead of two quantisation passes over it (dmy_fp8_quant).
# DMY_F8_DELAYED=0 keeps the just-in-time quantisation with the current amax.
F8_DELAYED = [os.environ.get('DMY_F8_DELAYED', '1') == '1']


# headroom on the delayed amax (DMY_F8_HEADROOM, >= 1; 1 = none): a margin against an activation range that grows
# between steps, at the cost of log2(headroom) bits of e4m3 resolution
F8_HEADROOM = [float(os.environ.get('DMY_F8_HEADROOM', '1'))]


class F8Emit:
    """Per producer layer: two ping-pong arrays of block maxima (this step's |y| maxima become the next step's
    quantisation amax) and the last call's per-block saturation counts.  The first step only records maxima (its
    consumer quantises just in time)."""
    __slots__ = ('buf', 'p', 'valid', 'numel')

    def __init__(self, dev):
        nb = call('dmy_bn_act_f8_blocks')
        self.buf = torch.zeros(3, nb, dtype=torch.float32, device=dev)
        self.p, self.valid, self.numel = 0, False, 0

    def run(self, z, scale, shift, act, res, rps, y, yps, M, K):
        """BN-act of the producer with the e4m3 side output; returns (y8, used amax) or None on the first step"""
        y8 = torch.empty(M * K, dtype=torch.uint8, device=z.device)
        used = f32(1, z.device)
        call('dmy_bn_act_fwd_f8', ptr(z), K, ptr(scale), ptr(shift), act, ptr(res), rps, ptr(y), yps, M, K, ptr(y8),
             ptr(self.buf[self.p]), ptr(self.buf[1 - self.p]), ptr(used), F8_HEADROOM[0], ptr(self.buf[2]), stream())
        self.p ^= 1
        out = (y8, used) if self.valid else None
        self.valid, self.numel = True, M * K
        return out

    def saturated(self):
        """(count, fraction) of the last call's e4m3 elements clipped at +-448 (a device sync)"""
        n = float(self.buf[2].sum()) if self.valid else 0.0
        return n, n / max(1, self.numel)


def _fp8_weight(weight, spec, wkey, dev):
    K, C, KH, KW = weight.shape
    fc = spec.f8cache
    if fc is not None and fc[0] == wkey:
        return fc[1], fc[2]
    w8 = torch.empty(weight.numel(), dtype=torch.uint8, device=dev)
    ws = f32(K, dev)
    call('dmy_conv_wprep_fp8', ptr(weight.detach().contiguous()), ptr(w8), ptr(ws), K, C, KH, KW, stream())
    spec.f8cache = (wkey, w8, ws)
    return w8, ws


def _fp8_operands(x, xps, weight, spec, wkey, f8in=None):
    """per-tensor e4m3 copy of the activation and the per-output-channel e4m3 weight (cached on the spec until the
    weight changes).  f8in = (x8, amax) emitted by the producer (delayed scaling), else dmy_fp8_quant with the
    current amax"""
    if f8in is not None:
        x8, amax = f8in
    else:
        N, C, H, W = x.shape
        rows = N * H * W
        x8 = torch.empty(rows * C, dtype=torch.uint8, device=x.device)
        amax = f32(_F8_WS[0] or _f8_ws(), x.device)  # [0] = the amax the quantisation used
        call('dmy_fp8_quant', ptr(x), rows, C, xps, ptr(x8), ptr(amax), stream())
    return (x8, amax, *_fp8_weight(weight, spec, wkey, x.device))


def _conv_fp8(x, g, weight, spec, wkey, f8in, prod, infer):
    """e4m3 operands (x8, amax, w8, wscale) when the layer runs on the fp8 kernel, else None.  f8in: the e4m3 copy the
    producer emitted with the input (delayed scaling); prod: the producer's spec, asked here to start emitting"""
    if not (spec.fp8 and g.groups == 1 and not g.s2d and g.Cp == g.C and fp8_eligible(g.C, g.K, x.dtype, g.N * g.H * g.W)):
        return None
    if f8in is not None and (f8in[0].numel() != g.N * g.H * g.W * g.C or not F8_DELAYED[0]):
        f8in = None
    f8 = _fp8_operands(x, g.xps, weight, spec, wkey, f8in)
    if f8in is None and prod is not None and prod.f8_emit is None and F8_DELAYED[0] and not infer:
        prod.f8_emit = F8Emit(x.device)  # from the next step on, the producer emits this input's e4m3 copy
    return f8
