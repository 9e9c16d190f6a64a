"""SPD-mix pieces (csrc/spd.hip; dmy_space_to_depth is csrc/eltwise.hip's): the 2 x 2 max pool, DMMConv2's SM / MP
split, plain space-to-depth, and the shape check of a conv layer followed by SM."""
import torch

from .._lib import call, ptr, stream
from ._base import VW, dcode, even_hw, new_act, out_or_new, pixel_stride, vec_check, vec_view
from .sinks import sink_result, sink_target


def _spd_shape(g, x, res):
    """output shape of an spd layer (N, 4K, OH / 2, OW / 2), after checking that the SM passes take it"""
    even_hw(g.OH, g.OW, 'a conv followed by SM')
    if res is not None:
        raise NotImplementedError('an spd conv layer takes no residual')
    if g.K % VW[x.dtype] or g.K // VW[x.dtype] > 256:
        raise NotImplementedError(f'the SM passes (csrc/spd.hip) take whole 16-byte vectors, at most 256 per pixel: '
                                  f'output channels multiples of {VW[x.dtype]} for {x.dtype}, got {g.K}')
    return g.N, 4 * g.K, g.OH // 2, g.OW // 2


class MaxPool2Fn(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) (MP, models/common.py:1469-1475): dmy_maxpool2_fwd keeps the window offset of each maximum,
    the backward gathers through it.  sink: the GradSink of x when x has other consumers (DMMConv)."""

    @staticmethod
    def forward(ctx, x, sink=None):
        dcode(x)
        x, xps = vec_view(x)
        N, C, H, W = x.shape
        vec_check('the 2 x 2 max pool (csrc/spd.hip)', x.dtype, [C], max_vecs=256)
        if H < 2 or W < 2:
            raise ValueError(f'MaxPool2d(2, 2) needs a map of at least 2 x 2, got {H}x{W}')
        y = new_act(N, C, H // 2, W // 2, x)
        arg = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
        call('dmy_maxpool2_fwd', dcode(x), ptr(x), xps, ptr(y), C, ptr(arg), N, H, W, C, stream())
        ctx.save_for_backward(arg)
        ctx.shape, ctx.sink = (N, C, H, W), sink
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dy, dps = vec_view(dy)
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, dy)
        call('dmy_maxpool2_bwd', dcode(dy), ptr(dy), dps, ptr(arg), ptr(buf), bps, acc, N, H, W, C, stream())
        return sink_result(ctx.sink, buf), None


class SpdSplitFn(torch.autograd.Function):
    """DMMConv2's front end (models/common.py:1516, 1519): one pass over x writes SM(x) into `out` (the first 4C
    channels of the module's concat buffer, or a fresh tensor) and MP(x) with its argmax; the backward is one launch,
    dx = SM^-1(d_sm) + the pool's gather of d_mp.  -> (sm, mp)"""

    @staticmethod
    def forward(ctx, x, out=None):
        dcode(x)
        x, xps = vec_view(x)
        N, C, H, W = x.shape
        even_hw(H, W, 'SM / DMMConv2')
        vec_check('the SM / MP split (csrc/spd.hip)', x.dtype, [C], max_vecs=256)
        sm, smps = out_or_new(out, (N, 4 * C, H // 2, W // 2), x)
        mp = new_act(N, C, H // 2, W // 2, x)
        arg = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
        call('dmy_spd_split_fwd', dcode(x), ptr(x), xps, ptr(sm), smps, ptr(mp), C, ptr(arg), N, H, W, C, stream())
        ctx.save_for_backward(arg)
        ctx.shape = (N, C, H, W)
        return sm, mp

    @staticmethod
    def backward(ctx, dsm, dmp):
        (arg,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dsm, dsps = vec_view(dsm)
        dmp, dmps = vec_view(dmp)
        dx = new_act(N, C, H, W, dsm)
        call('dmy_spd_split_bwd', dcode(dsm), ptr(dsm), dsps, ptr(dmp), dmps, ptr(arg), ptr(dx), C, N, H, W, C, stream())
        return dx, None


class SpaceToDepthFn(torch.autograd.Function):
    """models/common.py:1451-1458: cat(x[::2, ::2], x[1::2, ::2], x[::2, 1::2], x[1::2, 1::2]) on channels."""

    @staticmethod
    def forward(ctx, x):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y = new_act(N, 4 * C, H // 2, W // 2, x)
        call('dmy_space_to_depth', dcode(x), ptr(x), xps, ptr(y), 4 * C, N, H, W, C, 0, stream())
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.shape
        dy, dps = pixel_stride(dy)
        dx = new_act(N, C, H, W, dy)
        call('dmy_space_to_depth', dcode(dy), ptr(dx), C, ptr(dy), dps, N, H, W, C, 1, stream())
        return dx
