"""GnConv / HorBlock pieces (csrc/hor.hip): the gate product and the layer-scaled residual."""
import torch

from .._lib import call, ptr, stream
from ._base import CL, VW, dcode, f32, new_act, out_or_new, pixel_stride, vec_check
from .sinks import _write_target, pass_or_self


class GateMulFn(torch.autograd.Function):
    """y = a * b * scale: GnConv's gates `pwa * dw_list[0]`, `pws[i](x) * dw_list[i + 1]` with dw_abc's `* self.scale`
    (models/common.py:1349-1355).  a and b may be channel slices of wider buffers; the backward writes da / db in one
    launch into asink / bsink's targets (SliceSink parts: the slices of d(fused_x) / d(dw_abc))."""

    @staticmethod
    def forward(ctx, a, b, scale, asink=None, bsink=None, out=None):
        """out: None or [view] -- see out_view"""
        a, aps = pixel_stride(a)
        b, bps = pixel_stride(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f'GateMulFn: operands {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}')
        N, C, H, W = a.shape
        y, yps = out_or_new(out, (N, C, H, W), a)
        vec_check('GateMulFn', a.dtype, [C], [aps, bps, yps], [a, b, y])
        call('dmy_gate_fwd', dcode(a), ptr(a), aps, ptr(b), bps, ptr(y), yps, N * H * W, C, float(scale), stream())
        ctx.save_for_backward(a, b)
        ctx.ps, ctx.scale, ctx.asink, ctx.bsink = (aps, bps), float(scale), asink, bsink
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        aps, bps = ctx.ps
        N, C, H, W = a.shape
        dy, dps = pixel_stride(dy.to(a.dtype))
        da, daps, fa = _write_target(ctx.asink, N, C, H, W, a)
        db, dbps, fb = _write_target(ctx.bsink, N, C, H, W, a)
        vec_check('GateMulFn backward', a.dtype, [C], [dps, daps, dbps], [dy, da, db])
        call('dmy_gate_bwd', dcode(a), ptr(dy), dps, ptr(a), aps, ptr(b), bps, ptr(da), daps, ptr(db), dbps, N * H * W,
             C, ctx.scale, stream())
        return fa(), fb(), None, None, None, None


class LayerScaleAddFn(torch.autograd.Function):
    """out = x + gamma[c] * y: HorBlock's layer-scaled residuals (models/common.py:1388, 1395-1398, no DropPath).  The
    backward is one launch for dy = gamma * dout and the partial rows of dgamma = sum_m dout * y (summed in row order
    by dmy_reduce_rows); dx is dout itself, handed to xsink as a passthrough."""

    @staticmethod
    def forward(ctx, x, y, gamma, xsink=None, out=None):
        """out: None or [view] -- see out_view"""
        x, xps = pixel_stride(x)
        y = y.contiguous(memory_format=CL)
        N, C, H, W = x.shape
        if y.shape != x.shape or y.dtype != x.dtype or gamma.dtype != torch.float32 or gamma.numel() != C:
            raise ValueError(f'LayerScaleAddFn: x {tuple(x.shape)} {x.dtype}, y {tuple(y.shape)} {y.dtype}, gamma '
                             f'{tuple(gamma.shape)} {gamma.dtype}')
        gm = gamma.detach().contiguous()
        o, ops = out_or_new(out, (N, C, H, W), x)
        vec_check('LayerScaleAddFn', x.dtype, [C], [xps, ops], [x, y, o])
        call('dmy_layerscale_fwd', dcode(x), ptr(x), xps, ptr(y), ptr(gm), ptr(o), ops, N * H * W, C, stream())
        ctx.save_for_backward(y, gm)
        ctx.xsink = xsink
        return o

    @staticmethod
    def backward(ctx, dout):
        y, gm = ctx.saved_tensors
        N, C, H, W = y.shape
        M, dev = N * H * W, y.device
        dout, dps = pixel_stride(dout.to(y.dtype))
        vec_check('LayerScaleAddFn backward', y.dtype, [C], [dps], [dout])
        if C // VW[y.dtype] > 256:
            raise NotImplementedError(f'LayerScaleAddFn backward: {C} channels, at most {256 * VW[y.dtype]}')
        dy = new_act(N, C, H, W, y)
        P = call('dmy_layerscale_bwd_rows', M)
        part = f32(P * C, dev)
        call('dmy_layerscale_bwd', dcode(y), ptr(dout), dps, ptr(y), ptr(gm), ptr(dy), M, C, ptr(part), stream())
        dgamma = f32(C, dev)
        call('dmy_reduce_rows', ptr(part), P, C, ptr(dgamma), 0, stream())
        return pass_or_self(ctx.xsink, dout), dy, dgamma, None, None
