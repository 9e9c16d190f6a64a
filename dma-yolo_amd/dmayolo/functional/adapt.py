"""Adaptive-fusion necks (csrc/adapt.hip): AdaptConcat's gate, Adapt_Add2 / Adapt_Add3."""
import torch

from .._lib import call, ptr, stream
from ._base import dcode, f32, new_act, pixel_stride, vec_check
from .conv import WgradArena
from .sinks import sink_result, sink_target


def _lv3(xs, with_c=True):
    """(ptr, pixel stride[, channels]) argument triples of up to three levels, padded with nulls"""
    out = []
    for i in range(3):
        if i < len(xs):
            t, ps = xs[i]
            out += [ptr(t), ps] + ([t.shape[1]] if with_c else [])
        else:
            out += [None, 0] + ([0] if with_c else [])
    return out


class AdaptGateFn(torch.autograd.Function):
    """AdaptConcat's fusion (models/common.py:979-990): a = softmax(weight_levels(wm)) per pixel, y = cat(x_l * a_l).
    wm [N, 16 L, H, W] holds the level maps side by side; one launch forward, one backward (+ two row sums)."""

    @staticmethod
    def forward(ctx, W, b, sinks, wm, *xs):
        """sinks: None or one GradSink-or-None per input"""
        L = len(xs)
        if L not in (2, 3):
            raise NotImplementedError(f'AdaptConcat fuses 2 or 3 levels, got {L}')
        xs = [pixel_stride(x) for x in xs]
        wm, wmps = pixel_stride(wm)
        N, _, H, Wd = xs[0][0].shape
        chans = [x.shape[1] for x, _ in xs]
        if wm.shape[1] != 16 * L or tuple(W.shape[:2]) != (L, 16 * L):
            raise NotImplementedError('AdaptConcat: 16 level-map channels per level (rfb=False)')
        M, Ct = N * H * Wd, sum(chans)
        y = new_act(N, Ct, H, Wd, wm)
        vec_check('AdaptConcat', wm.dtype, chans, [ps for _, ps in xs] + [wmps], [x for x, _ in xs] + [wm])
        a = f32(M * L, wm.device)
        Wc, bc = W.detach().contiguous(), b.detach().contiguous()
        call('dmy_adapt_gate_fwd', dcode(wm), L, *_lv3(xs), ptr(wm), wmps, ptr(Wc), ptr(bc), ptr(y), Ct, ptr(a), M,
             stream())
        ctx.save_for_backward(Wc, wm, a, *[x for x, _ in xs])
        ctx.sinks, ctx.arena, ctx.keys = sinks, WgradArena.current, (W.data_ptr(), b.data_ptr())
        ctx.wshape = tuple(W.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        Wc, wm, a, *xs = ctx.saved_tensors
        L = len(xs)
        xs = [pixel_stride(x) for x in xs]
        wm, wmps = pixel_stride(wm)
        dy, dps = pixel_stride(dy.to(wm.dtype))
        N, Ct, H, Wd = dy.shape
        M, dev = N * H * Wd, dy.device
        sinks = ctx.sinks or [None] * L
        tg = [sink_target(sinks[l], N, x.shape[1], H, Wd, dy) for l, (x, _) in enumerate(xs)]
        acc = sum(t[2] << l for l, t in enumerate(tg))
        vec_check('AdaptConcat backward', wm.dtype, [], [dps] + [t[1] for t in tg], [dy] + [t[0] for t in tg])
        dwm = new_act(N, 16 * L, H, Wd, wm)
        nb = call('dmy_adapt_gate_blocks', dcode(wm), M, Ct, L)
        pdw, pdb = f32(nb * L * 16 * L, dev), f32(nb * L, dev)
        dxa = []
        for l in range(3):
            dxa += [ptr(tg[l][0]), tg[l][1]] if l < L else [None, 0]
        call('dmy_adapt_gate_bwd', dcode(wm), L, ptr(dy), dps, *_lv3(xs), ptr(a), ptr(wm), wmps, ptr(Wc), *dxa, acc,
             ptr(dwm), 16 * L, ptr(pdw), ptr(pdb), M, stream())
        # the partial rows, summed in row order (deterministic)
        dW = ctx.arena.take(ctx.keys[0], ctx.wshape) if ctx.arena is not None else None
        db = ctx.arena.take(ctx.keys[1], (L,)) if ctx.arena is not None else None
        dW = dW if dW is not None else torch.empty(ctx.wshape, dtype=torch.float32, device=dev)
        db = db if db is not None else f32(L, dev)
        call('dmy_reduce_rows', ptr(pdw), nb, L * 16 * L, ptr(dW), 0, stream())
        call('dmy_reduce_rows', ptr(pdb), nb, L, ptr(db), 0, stream())
        grads = [sink_result(sinks[l], tg[l][0]) for l in range(L)]
        return (dW, db, None, dwm, *grads)


class AdaptAddFn(torch.autograd.Function):
    """Adapt_Add2 / Adapt_Add3's fusion (models/common.py:1040-1044, 1057-1061): y = silu(sum_i w_i / (sum w + eps) *
    x_i) over 2 or 3 inputs of equal shape; the backward recomputes the sum from the inputs."""

    @staticmethod
    def forward(ctx, w, eps, sinks, *xs):
        n = len(xs)
        if n not in (2, 3) or len({tuple(x.shape) for x in xs}) != 1:
            raise NotImplementedError(f'Adapt_Add: 2 or 3 inputs of one shape, got {[tuple(x.shape) for x in xs]}')
        xs = [pixel_stride(x) for x in xs]
        x0 = xs[0][0]
        N, C, H, Wd = x0.shape
        vec_check('Adapt_Add', x0.dtype, [C], [ps for _, ps in xs], [x for x, _ in xs])
        y = new_act(N, C, H, Wd, x0)
        wc = w.detach().contiguous()
        call('dmy_adapt_add_fwd', dcode(x0), n, *_lv3(xs, False), ptr(wc), float(eps), ptr(y), C, N * H * Wd, C,
             stream())
        ctx.save_for_backward(wc, *[x for x, _ in xs])
        ctx.sinks, ctx.eps = sinks, float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        wc, *xs = ctx.saved_tensors
        n = len(xs)
        xs = [pixel_stride(x) for x in xs]
        dy, dps = pixel_stride(dy.to(xs[0][0].dtype))
        N, C, H, Wd = dy.shape
        M = N * H * Wd
        sinks = ctx.sinks or [None] * n
        tg = [sink_target(sinks[i], N, C, H, Wd, dy) for i in range(n)]
        acc = sum(t[2] << i for i, t in enumerate(tg))
        vec_check('Adapt_Add backward', dy.dtype, [], [dps] + [t[1] for t in tg], [dy] + [t[0] for t in tg])
        nb = call('dmy_dot_partial_blocks', M, C)
        part = f32(n * nb, dy.device)
        dxa = []
        for i in range(3):
            dxa += [ptr(tg[i][0]), tg[i][1]] if i < n else [None, 0]
        call('dmy_adapt_add_bwd', dcode(dy), n, ptr(dy), dps, *_lv3(xs, False), ptr(wc), ctx.eps, *dxa, acc, ptr(part),
             M, C, stream())
        dw = torch.empty_like(wc)
        call('dmy_bifpn_wgrad', ptr(part), nb, n, ptr(wc), ctx.eps, ptr(dw), stream())
        grads = [sink_result(sinks[i], tg[i][0]) for i in range(n)]
        return (dw, None, None, *grads)
