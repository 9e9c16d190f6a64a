"""Pooling, nearest resize, concat and add (csrc/eltwise.hip)."""
import torch

from .._lib import call, ptr, stream
from ._base import CL, VW, ctypes_off, dcode, new_act, out_or_new, out_view, pixel_stride, vec_ok
from .sinks import pass_or_self, sink_result, sink_target


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, sink=None, out=None):
        """out: None or [view] -- a concat_buffer channel slice the pooled map is written into (SPPF / SPPFCSPC), in a
        list so autograd does not treat the buffer as an input"""
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y, yps = out_or_new(out, (N, C, H, W), x)
        arg = torch.empty((N, H, W, C), dtype=torch.uint8, device=x.device)
        call('dmy_maxpool_fwd', dcode(x), ptr(x), xps, ptr(y), yps, ptr(arg), N, H, W, C, k, stream())
        ctx.save_for_backward(arg)
        ctx.k, ctx.shape, ctx.sink = k, (N, C, H, W), sink
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dy, dps = pixel_stride(dy)
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, dy)
        call('dmy_maxpool_bwd', dcode(dy), ptr(dy), dps, ptr(arg), ptr(buf), bps, acc, N, H, W, C, ctx.k, stream())
        return sink_result(ctx.sink, buf), None, None, None


def maxpool_chain3(x, k, outs=(None, None, None)):
    """inference SPPF / SPPFCSPC pyramid: (pool(x), pool(pool(x)), pool(pool(pool(x)))) with the k x k stride-1 pool in
    ONE launch (dmy_maxpool_chain3_fwd, the bits of three MaxPoolFn launches), written into `outs` when they are three
    NHWC views with one pixel stride (concat_buffer slices), else into fresh tensors.  None when autograd is recording
    (the backward needs MaxPoolFn's argmax) or the kernel does not take the shape: the caller chains MaxPoolFn"""
    if torch.is_grad_enabled() or k not in (3, 5) or x.dtype not in (torch.bfloat16, torch.float32):
        return None
    x, xps = pixel_stride(x)
    N, C, H, W = x.shape
    vw = VW[x.dtype]
    views = [out_view(o, (N, C, H, W), x) for o in outs]
    yps = views[0][1]
    if yps is not None and all(ps == yps for _, ps in views):  # three valid views with one pixel stride
        ys = [v for v, _ in views]
    else:
        ys, yps = [new_act(N, C, H, W, x) for _ in range(3)], C
    if not vec_ok(x.dtype, [C], [xps, yps], [x] + ys) or N * (C // vw) >= 65536:
        return None
    call('dmy_maxpool_chain3_fwd', dcode(x), ptr(x), xps, ptr(ys[0]), ptr(ys[1]), ptr(ys[2]), yps, N, H, W, C, k,
         stream())
    return tuple(ys)


class AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, sink=None):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y = new_act(N, C, H // r, W // r, x)
        call('dmy_avgpool_fwd', dcode(x), ptr(x), xps, ptr(y), N, H, W, C, r, stream())
        ctx.r, ctx.shape, ctx.sink = r, (N, C, H, W), sink
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.shape
        dy = dy.contiguous(memory_format=CL)
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, dy)
        call('dmy_avgpool_bwd', dcode(dy), ptr(dy), ptr(buf), bps, acc, N, H, W, C, ctx.r, stream())
        return sink_result(ctx.sink, buf), None, None


class ResizeFn(torch.autograd.Function):
    """nearest resize with ATen's index rule (F.interpolate(mode='nearest'), nn.Upsample)."""

    @staticmethod
    def forward(ctx, x, OH, OW, out=None):
        """out: None or [view] -- a concat_buffer channel slice the result is written into (Model's concat plan)"""
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y, yps = out_or_new(out, (N, C, OH, OW), x)
        call('dmy_resize_fwd', dcode(x), ptr(x), xps, ptr(y), yps, 1.0, N, H, W, OH, OW, C, stream())
        ctx.shape = (N, C, H, W, OH, OW)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, OH, OW = ctx.shape
        dy, dps = pixel_stride(dy)
        dx = new_act(N, C, H, W, dy)
        call('dmy_resize_bwd', dcode(dy), ptr(dy), dps, ptr(dx), C, N, H, W, OH, OW, C, stream())
        return dx, None, None, None


class ConcatFn(torch.autograd.Function):
    """cat(w_i/(sum w + eps) * x_i) along channels (w=None: plain Concat)."""

    @staticmethod
    def forward(ctx, w, eps, sinks, *xs):
        """sinks: None or one GradSink-or-None per input (the slice gradient is handed to it)"""
        ctx.sinks = sinks
        base = _inplace_concat(xs) if w is None else None
        xs = [pixel_stride(x) for x in xs]
        N, _, H, W = xs[0][0].shape
        Ct = sum(x.shape[1] for x, _ in xs)
        y = base.detach() if base is not None else new_act(N, Ct, H, W, xs[0][0])
        c0 = 0
        M = N * H * W
        for i, (x, xps) in enumerate(xs):
            if base is not None:  # the producers wrote their slices in place (concat_buffer)
                break
            C = x.shape[1]
            call('dmy_slice_copy', dcode(x), ptr(x), xps, ctypes_off(y, c0), Ct, M, C, ptr(w), i,
                 len(xs) if w is not None else 0, float(eps), 0, stream())
            c0 += C
        ctx.chans = [x.shape[1] for x, _ in xs]
        ctx.eps = eps
        if w is not None:
            ctx.save_for_backward(w, *[x for x, _ in xs])
        else:
            ctx.save_for_backward()
        ctx.has_w = w is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, dps = pixel_stride(dy)
        N, Ct, H, W = dy.shape
        M = N * H * W
        grads, c0 = [], 0
        sinks = ctx.sinks or [None] * len(ctx.chans)
        if not ctx.has_w:
            for C, sk in zip(ctx.chans, sinks):
                sl = dy[:, c0:c0 + C]
                grads.append(pass_or_self(sk, sl))
                c0 += C
            return (None, None, None, *grads)
        w, *xs = ctx.saved_tensors
        nb = call('dmy_dot_partial_blocks', M, max(ctx.chans))
        part = torch.zeros((len(xs), nb), dtype=torch.float32, device=dy.device)
        for i, (x, C) in enumerate(zip(xs, ctx.chans)):
            x, xps = pixel_stride(x)
            g, gps, acc = sink_target(sinks[i], N, C, H, W, dy)
            sl = dy[:, c0:c0 + C]
            if vec_ok(dy.dtype, [C], [dps, gps, xps], [sl, g, x]):  # one pass over the dy slice
                call('dmy_slice_copy_dot', dcode(dy), ptr(sl), dps, ptr(g), gps, ptr(x), xps, M, C, ptr(w), i, len(xs),
                     float(ctx.eps), acc, ptr(part[i]), stream())
            else:
                call('dmy_slice_copy', dcode(dy), ptr(sl), dps, ptr(g), gps, M, C, ptr(w), i, len(xs), float(ctx.eps),
                     acc, stream())
                call('dmy_dot_partial', dcode(dy), ptr(sl), dps, ptr(x), xps, M, C, ptr(part[i]), stream())
            g = sink_result(sinks[i], g)
            nbi = call('dmy_dot_partial_blocks', M, C)
            if nbi < nb:
                part[i, nbi:].zero_()
            grads.append(g)
            c0 += C
        dw = torch.empty_like(w)
        call('dmy_bifpn_wgrad', ptr(part), nb, len(xs), ptr(w), float(ctx.eps), ptr(dw), stream())
        return (dw, None, None, *grads)


def _inplace_concat(xs):
    """the concat_buffer whose consecutive channel slices the inputs are, in order, or None"""
    b = xs[0]._base
    if b is None or b.dim() != 4 or not b.is_contiguous(memory_format=CL):
        return None
    N, Ct, H, W = b.shape
    c0, es = 0, b.element_size()
    for x in xs:
        if x._base is not b or x.shape[0] != N or x.shape[2:] != b.shape[2:] or \
                x.data_ptr() != b.data_ptr() + c0 * es or x.stride() != b.stride():
            return None
        c0 += x.shape[1]
    return b if c0 == Ct else None


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, asink=None):
        ctx.asink = asink
        a = a.contiguous(memory_format=CL) if a.dim() == 4 else a.contiguous()
        b = b.contiguous(memory_format=CL) if b.dim() == 4 else b.contiguous()
        y = torch.empty_like(a)
        call('dmy_pointwise', dcode(a), 0, 0, ptr(a), ptr(b), ptr(y), a.numel(), 1.0, stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return pass_or_self(ctx.asink, dy), dy, None
