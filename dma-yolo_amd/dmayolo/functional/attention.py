"""Gating and attention glue (csrc/eltwise.hip): SCConv's gate, CoorAttention's pool / apply, CBAM's pieces
(models/common.py:260-310)."""
import torch

from .._lib import call, ptr, stream
from ._base import CL, dcode, f32, new_act, pixel_stride
from .sinks import pass_or_self, sink_result, sink_target


class SCGateFn(torch.autograd.Function):
    """out = u3 * sigmoid(x + nearest(g))  (models/common.py:1311-1314).  When u3 is k3's deferred BN output (z with
    `_dmy_affine`, conv_bn_act(defer=True)), the gate applies k3's BN scale / shift to z itself and its backward writes
    k3's BN backward-reduce partials into k3's BnLink (dmy_scgate_bn_fwd / _bwd), so k3's bn_act_fwd and
    bn_bwd_reduce passes disappear."""

    @staticmethod
    def forward(ctx, x, u3, g, sink=None):
        ctx.sink = sink
        aff, link = getattr(u3, '_dmy_affine', None), getattr(u3, '_dmy_bnlink', None)
        x, xps = pixel_stride(x)
        g = g.contiguous(memory_format=CL)
        N, C, H, W = x.shape
        GH, GW = g.shape[2:]
        out = new_act(N, C, H, W, x)
        ctx.aff = ctx.link = None
        if aff is not None:
            assert pixel_stride(u3)[0] is u3 and u3.stride(1) == 1 and u3.stride(3) == C, 'deferred z must be dense NHWC'
            call('dmy_scgate_bn_fwd', ptr(x), xps, ptr(u3), ptr(aff[0]), ptr(aff[1]), ptr(g), ptr(out), N, H, W, C, GH,
                 GW, stream())
            ctx.aff, ctx.link = aff, link
        else:
            u3 = u3.contiguous(memory_format=CL)
            call('dmy_scgate_fwd', dcode(x), ptr(x), xps, ptr(u3), ptr(g), ptr(out), N, H, W, C, GH, GW, stream())
        ctx.save_for_backward(x, u3, g)
        ctx.xps = xps
        return out

    @staticmethod
    def backward(ctx, dout):
        x, u3, g = ctx.saved_tensors
        N, C, H, W = x.shape
        GH, GW = g.shape[2:]
        dout = dout.contiguous(memory_format=CL)
        du3 = new_act(N, C, H, W, x)
        # d(x + up(g)) -> x's gradient sink; the resize backward of g needs it on its own
        dpre = new_act(N, C, H, W, x)
        if ctx.aff is not None:
            sc, sh, mean, invstd = ctx.aff
            P = call('dmy_scgate_bn_rows', N, H, W, C)
            pdb, pdg = f32(P * C, x.device), f32(P * C, x.device)
            call('dmy_scgate_bn_bwd', ptr(x), ctx.xps, ptr(u3), ptr(sc), ptr(sh), ptr(mean), ptr(invstd), ptr(g),
                 ptr(dout), ptr(du3), ptr(dpre), N, H, W, C, GH, GW, ptr(pdb), ptr(pdg), stream())
            # k3's ConvBNActFn backward takes these partials iff the gradient it receives IS du3, unmodified
            ctx.link.ready = (du3, C, pdb, pdg, P, du3._version)
        else:
            call('dmy_scgate_bwd', dcode(x), ptr(x), ctx.xps, ptr(u3), ptr(g), ptr(dout), ptr(du3), ptr(dpre), C, 0,
                 N, H, W, C, GH, GW, stream())
        dg = new_act(N, C, GH, GW, x)
        call('dmy_resize_bwd', dcode(x), ptr(dpre), C, ptr(dg), C, N, GH, GW, H, W, C, stream())
        return pass_or_self(ctx.sink, dpre), du3, dg, None


class CAPoolFn(torch.autograd.Function):
    """[N,C,H,W] -> [N,C,H+W,1]: row means then column means (CoorAttention pool_h / pool_w + cat)."""

    @staticmethod
    def forward(ctx, x):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        y = new_act(N, C, H + W, 1, x)
        call('dmy_ca_pool_fwd', dcode(x), ptr(x), xps, ptr(y), N, H, W, C, stream())
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.shape
        dy = dy.contiguous(memory_format=CL)
        dx = new_act(N, C, H, W, dy)
        call('dmy_ca_pool_bwd', dcode(dy), ptr(dy), ptr(dx), C, 0, N, H, W, C, stream())
        return dx


class CAApplyFn(torch.autograd.Function):
    """out = x * sigmoid(lw)[w] * sigmoid(lh)[h]; lh/lw are conv_h/conv_w logits over all H+W rows."""

    @staticmethod
    def forward(ctx, x, lh, lw):
        x, xps = pixel_stride(x)
        lh = lh.contiguous(memory_format=CL)
        lw = lw.contiguous(memory_format=CL)
        N, C, H, W = x.shape
        out = new_act(N, C, H, W, x)
        call('dmy_ca_apply_fwd', dcode(x), ptr(x), xps, ptr(lh), ptr(lw), ptr(out), C, N, H, W, C, stream())
        ctx.save_for_backward(x, lh, lw)
        ctx.xps = xps
        return out

    @staticmethod
    def backward(ctx, dout):
        x, lh, lw = ctx.saved_tensors
        N, C, H, W = x.shape
        dout, dps = pixel_stride(dout)
        dx = new_act(N, C, H, W, x)
        dlh = torch.empty_like(lh)
        dlw = torch.empty_like(lw)
        call('dmy_ca_apply_bwd', dcode(x), ptr(x), ctx.xps, ptr(lh), ptr(lw), ptr(dout), dps, ptr(dx), C, ptr(dlh),
             ptr(dlw), N, H, W, C, stream())
        return dx, dlh, dlw


class GPoolFn(torch.autograd.Function):
    """[N,C,H,W] -> [2N,C,1,1]: global average pool rows, then global max pool rows (first max)."""

    @staticmethod
    def forward(ctx, x, sink=None):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        z = new_act(2 * N, C, 1, 1, x)
        arg = torch.empty((N, C), dtype=torch.int32, device=x.device)
        ws = torch.empty(call('dmy_gpool_ws_bytes', dcode(x), N, H * W, C) // 4, dtype=torch.float32, device=x.device)
        call('dmy_gpool_fwd', dcode(x), ptr(x), xps, N, H * W, C, ptr(z), ptr(arg), ptr(ws), stream())
        ctx.save_for_backward(arg)
        ctx.shape, ctx.sink = (N, C, H, W), sink
        return z

    @staticmethod
    def backward(ctx, dz):
        (arg,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dz = dz.contiguous()
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, dz)
        call('dmy_gpool_bwd', dcode(dz), ptr(dz), ptr(arg), ptr(buf), bps, acc, N, H * W, C, stream())
        return sink_result(ctx.sink, buf), None


class HalvesSigmoidFn(torch.autograd.Function):
    """[2N,C,1,1] -> [N,C,1,1]: sigmoid(z[:N] + z[N:]) (CBAM channel attention: sigmoid(avgout + maxout))."""

    @staticmethod
    def forward(ctx, z):
        z = z.contiguous()
        N2, C = z.shape[:2]
        ca = torch.empty((N2 // 2, C, 1, 1), dtype=z.dtype, device=z.device)
        call('dmy_halves_sigmoid', dcode(z), ptr(z), N2 // 2, C, ptr(ca), None, None, stream())
        ctx.save_for_backward(z)
        return ca

    @staticmethod
    def backward(ctx, dca):
        (z,) = ctx.saved_tensors
        N2, C = z.shape[:2]
        dca = dca.contiguous()
        dz = torch.empty_like(z)
        call('dmy_halves_sigmoid', dcode(z), ptr(z), N2 // 2, C, None, ptr(dca), ptr(dz), stream())
        return dz


class CBAMInFn(torch.autograd.Function):
    """(x, ca) -> out1 = ca * x and s2 = cat(mean_c out1, max_c out1) (CBAM spatial-attention input)."""

    @staticmethod
    def forward(ctx, x, ca, sink=None):
        x, xps = pixel_stride(x)
        N, C, H, W = x.shape
        ca = ca.contiguous()
        out1 = new_act(N, C, H, W, x)
        s2 = new_act(N, 2, H, W, x)
        am = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
        call('dmy_cbam_in_fwd', dcode(x), ptr(x), xps, ptr(ca), N, H * W, C, ptr(out1), ptr(s2), ptr(am), stream())
        ctx.save_for_backward(x, ca, am)
        ctx.xps, ctx.sink = xps, sink
        return out1, s2

    @staticmethod
    def backward(ctx, dout1, ds2):
        x, ca, am = ctx.saved_tensors
        N, C, H, W = x.shape
        if dout1 is None:
            dout1 = torch.zeros_like(x)
        dout1, dps = pixel_stride(dout1)
        ds2 = torch.zeros((N, 2, H, W), dtype=x.dtype, device=x.device, memory_format=CL) if ds2 is None else \
            ds2.contiguous(memory_format=CL)
        buf, bps, acc = sink_target(ctx.sink, N, C, H, W, x)
        dca = f32(N * C, x.device)
        ws = f32(call('dmy_cbam_in_bwd_ws_elems', N, H * W, C), x.device)  # per-wave partials, folded in order
        call('dmy_cbam_in_bwd', dcode(x), ptr(x), ctx.xps, ptr(ca), ptr(dout1), dps, ptr(ds2), ptr(am), N, H * W, C,
             ptr(buf), bps, acc, ptr(dca), ptr(ws), stream())
        return sink_result(ctx.sink, buf), dca.view(N, C, 1, 1).to(ca.dtype), None


class PixScaleFn(torch.autograd.Function):
    """out = out1 * sa, sa one value per pixel [N,1,H,W] (CBAM: spatial_attention(out) * out)."""

    @staticmethod
    def forward(ctx, out1, sa):
        out1 = out1.contiguous(memory_format=CL)
        sa, sps = pixel_stride(sa)
        N, C, H, W = out1.shape
        out = new_act(N, C, H, W, out1)
        call('dmy_pixscale', dcode(out1), ptr(out1), ptr(sa), sps, N, H * W, C, ptr(out), C, None, 0, None, None,
             stream())
        ctx.save_for_backward(out1, sa)
        ctx.sps = sps
        return out

    @staticmethod
    def backward(ctx, dout):
        out1, sa = ctx.saved_tensors
        N, C, H, W = out1.shape
        dout, dps = pixel_stride(dout)
        dout1 = new_act(N, C, H, W, out1)
        dsa = new_act(N, 1, H, W, out1)
        call('dmy_pixscale', dcode(out1), ptr(out1), ptr(sa), ctx.sps, N, H * W, C, None, 0, ptr(dout), dps,
             ptr(dout1), ptr(dsa), stream())
        return dout1, dsa
