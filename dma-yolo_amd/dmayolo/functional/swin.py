"""Transformer pieces: LayerNorm, window attention, dropout / drop-path (csrc/swin.hip), global attention
(csrc/mha.hip) and TDetect's level flatten (csrc/tal.hip)."""
import torch

from .._lib import call, ptr, stream
from ._base import CL, dcode, f32, new_act, pixel_stride
from .sinks import pass_or_self, sink_result, sink_target


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over channels of an NHWC activation (common.py:560, 565)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, sink=None):
        ctx.sink = sink
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        M = N * H * W
        y = new_act(N, C, H, W, x)
        mean, rstd = f32(M, x.device), f32(M, x.device)
        call('dmy_layernorm_fwd', dcode(x), ptr(x), xps, ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, C,
             float(eps), stream())
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.xps = xps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        N, C, H, W = x.shape
        M = N * H * W
        dy, dps = pixel_stride(dy)
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, x)
        P = call('dmy_layernorm_bwd_blocks', M)
        pdw, pdb = f32(P * C, x.device), f32(P * C, x.device)
        call('dmy_layernorm_bwd', dcode(x), ptr(x), ctx.xps, ptr(dy), dps, ptr(w), ptr(mean), ptr(rstd), ptr(buf), bps,
             acc, M, C, ptr(pdw), ptr(pdb), stream())
        dx = sink_result(ctx.sink, buf)
        dw, db = f32(C, x.device), f32(C, x.device)
        call('dmy_reduce_rows', ptr(pdw), P, C, ptr(dw), 0, stream())
        call('dmy_reduce_rows', ptr(pdb), P, C, ptr(db), 0, stream())
        return dx, dw, db, None, None


class WinAttnFn(torch.autograd.Function):
    """Shifted-window MHSA core (common.py:500-545 + 595-631): qkv [N,3C,H,W] NHWC -> [N,C,H,W]."""

    @staticmethod
    def forward(ctx, qkv, table, nh, shift, scale):
        qkv = qkv.contiguous(memory_format=CL)
        N, C3, H, W = qkv.shape
        C = C3 // 3
        out = torch.empty((N, C, H, W), dtype=qkv.dtype, device=qkv.device, memory_format=CL)  # every pixel is written
        tab = table.detach().float().contiguous()
        call('dmy_winattn_fwd', dcode(qkv), ptr(qkv), ptr(tab), ptr(out), N, H, W, C, nh, shift, float(scale),
             stream())
        ctx.save_for_backward(qkv, tab)
        ctx.cfg = (nh, shift, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, tab = ctx.saved_tensors
        nh, shift, scale = ctx.cfg
        N, C3, H, W = qkv.shape
        dout = dout.contiguous(memory_format=CL)
        dqkv = torch.empty_like(qkv, memory_format=CL)  # every pixel belongs to exactly one window
        groups = call('dmy_winattn_bwd_groups', N, H, W, nh)
        part = f32(groups * nh * 225, qkv.device)
        dtab = torch.empty_like(tab)
        call('dmy_winattn_bwd', dcode(qkv), ptr(qkv), ptr(dout), ptr(tab), ptr(dqkv), ptr(part), ptr(dtab), N, H, W,
             C3 // 3, nh, shift, float(scale), stream())
        return dqkv, dtab, None, None, None


class MHAFn(torch.autograd.Function):
    """Global multi-head attention core of nn.MultiheadAttention (common.py:323, C3TR): q, k, v are the
    in-projected NHWC token tensors [N, c, H, W] (tokens = the H*W pixels of one image); returns
    softmax(q k^T / sqrt(d)) v per head, [N, c, H, W].  Kernels: csrc/mha.hip (flash-style, nothing
    L x L is stored; the backward recomputes P from the saved log-sum-exp)."""

    @staticmethod
    def forward(ctx, q, k, v, nh):
        q, qps = pixel_stride(q)
        k, kps = pixel_stride(k)
        v, vps = pixel_stride(v)
        N, C, H, W = q.shape
        assert C % nh == 0 and k.shape == q.shape and v.shape == q.shape
        d, L = C // nh, H * W
        o = new_act(N, C, H, W, q)
        lse = f32(N * nh * L, q.device)
        call('dmy_mha_fwd', dcode(q), ptr(q), qps, ptr(k), kps, ptr(v), vps, ptr(o), C, ptr(lse), N, L, nh, d,
             float(d) ** -0.5, stream())
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.ps, ctx.nh = (qps, kps, vps), nh
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        qps, kps, vps = ctx.ps
        N, C, H, W = q.shape
        nh = ctx.nh
        d, L = C // nh, H * W
        do = do.to(q.dtype).contiguous(memory_format=CL)
        dq, dk, dv = new_act(N, C, H, W, q), new_act(N, C, H, W, q), new_act(N, C, H, W, q)
        Dq = f32(N * nh * L, q.device)
        call('dmy_mha_bwd', dcode(q), ptr(q), qps, ptr(k), kps, ptr(v), vps, ptr(o), ptr(do), C, ptr(lse), ptr(Dq),
             ptr(dq), ptr(dk), ptr(dv), N, L, nh, d, float(d) ** -0.5, stream())
        return dq, dk, dv, None


_DROP_STATE = {}


def _seed(dev):
    """A fresh dropout seed in device memory: dmy_dropout_seed advances a per-device generator state (seeded
    once from torch's CPU generator) on the stream, so a HIP-graph replay of the step draws a new mask each
    time instead of replaying the captured one.  Returns the [1] int64 seed tensor the kernels read."""
    st = _DROP_STATE.get(dev)
    if st is None:
        st = _DROP_STATE[dev] = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(dev)
    seed = torch.empty(1, dtype=torch.int64, device=dev)
    call('dmy_dropout_seed', ptr(st), ptr(seed), stream())
    return seed


class DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in train mode (common.py:328): y = x * keep / (1 - p); the keep mask is a counter
    hash of (seed, element index), regenerated in the backward from the same device-resident seed."""

    @staticmethod
    def forward(ctx, x, p):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y = new_act(N, C, H, W, x)
        seed = _seed(x.device)
        call('dmy_dropout', dcode(x), ptr(x), xps, ptr(y), C, N * H * W, C, float(p), ptr(seed), stream())
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, dps = pixel_stride(dy)
        N, C, H, W = dy.shape
        dx = new_act(N, C, H, W, dy)
        call('dmy_dropout', dcode(dy), ptr(dy), dps, ptr(dx), C, N * H * W, C, float(ctx.p), ptr(ctx.seed), stream())
        return dx, None


def _sample_major(t):
    """a layout in which each sample (dim 0) is one contiguous block: NHWC for 4-D activations, else row-major"""
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


class SampleScaleFn(torch.autograd.Function):
    """y = x * s[b] (DropPath with a pre-drawn per-sample keep mask, common.py:386-403), any rank."""

    @staticmethod
    def forward(ctx, x, s):
        x = _sample_major(x)
        y = torch.empty_like(x)  # preserve_format: same strides as x
        call('dmy_sample_scale', dcode(x), ptr(x), ptr(s), ptr(y), x.numel() // x.shape[0], x.numel(), stream())
        ctx.save_for_backward(s)
        return y

    @staticmethod
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        dy = _sample_major(dy)
        dx = torch.empty_like(dy)
        call('dmy_sample_scale', dcode(dy), ptr(dy), ptr(s), ptr(dx), dy.numel() // dy.shape[0], dy.numel(), stream())
        return dx, None


class DropPathAddFn(torch.autograd.Function):
    """x + DropPath(f) (common.py:386-403 with the residual of common.py:621-627): y = x + f * s[b], s[b] = floor(keep +
    u[b]) / keep on torch's drawn uniforms u [N] (csrc/swin.hip droppath_add_kernel: one pass, one rounding of the sum;
    was dmy_sample_scale + AddFn + torch's floor / div).  Backward: dx = dy (through the residual's GradSink when it
    has one), df = dy * s[b]."""

    @staticmethod
    def forward(ctx, x, f, u, keep, xsink=None):
        x, f = _sample_major(x), _sample_major(f)
        assert x.shape == f.shape and u.numel() == x.shape[0] and u.dtype == torch.float32
        y = torch.empty_like(x)
        call('dmy_droppath_add', dcode(x), ptr(x), ptr(f), ptr(u), float(keep), ptr(y), x.numel() // x.shape[0],
             x.numel(), stream())
        ctx.save_for_backward(u)
        ctx.keep, ctx.xsink = float(keep), xsink
        return y

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        dy = _sample_major(dy)
        df = torch.empty_like(dy)
        call('dmy_droppath_grad', dcode(dy), ptr(dy), ptr(u), ctx.keep, ptr(df), dy.numel() // dy.shape[0], dy.numel(),
             stream())
        return pass_or_self(ctx.xsink, dy), df, None, None, None


class FlattenLevelsFn(torch.autograd.Function):
    """TDetect (models/detect_t.py:45-47): per-level NHWC head outputs [B, no, H, W] -> one
    anchor-major [B, A, no] tensor (levels in order, anchors row-major within a level)."""

    @staticmethod
    def forward(ctx, *xs):
        B, no = xs[0].shape[:2]
        A = sum(x.shape[2] * x.shape[3] for x in xs)
        F = torch.empty((B, A, no), dtype=xs[0].dtype, device=xs[0].device)
        a0 = 0
        geo = []
        for x in xs:
            x, xps = pixel_stride(x)
            H, W = x.shape[2:]
            call('dmy_tal_flatten', dcode(x), ptr(x), xps, B, H, W, A, a0, no, ptr(F), 0, stream())
            geo.append((H, W, a0))
            a0 += H * W
        ctx.geo, ctx.B, ctx.no, ctx.A = geo, B, no, A
        return F

    @staticmethod
    def backward(ctx, dF):
        dF = dF.contiguous()
        out = []
        for H, W, a0 in ctx.geo:
            dx = new_act(ctx.B, ctx.no, H, W, dF)
            call('dmy_tal_flatten', dcode(dF), ptr(dx), ctx.no, ctx.B, H, W, ctx.A, a0, ctx.no, ptr(dF), 1, stream())
            out.append(dx)
        return tuple(out)
