"""conv -> act -> BN (+ residual): the activation BEFORE the BatchNorm (ConvMix, models/cspcm.py:28-37), over
csrc/convmix.hip and the conv engine's launches."""
import torch

from .._lib import call, ptr, stream, ACT_NONE
from ._base import VW, const_vec, dcode, f32, new_act, out_or_new, vec_ok, vec_view
from .conv import _bn_bwd_finalize, _bn_finalize, _bn_sync, _conv_operands, _conv_wgrad, _dgrad, _dw_check, \
    _fold_partials, _launch_conv_fwd, _param_spec, _pgrad, _save_ctx, eval_coef
from .sinks import pass_or_self
from .timer import KernelTimer


def _actbn_stats(z, g, spec, bn, train_bn, sync=None):
    """BN coefficients over a = act(z) -> (scale, shift, mean, invstd).  Train mode: dmy_actbn_stats' partial rows,
    folded and finalized by the unchanged dmy_bn_finalize (which also updates the running statistics); eval-mode BN
    under autograd: scale / shift from the running statistics, mean / invstd unused (zero / one)."""
    K, M, dev = g.K, g.M, z.device
    scale, shift = f32(K, dev), f32(K, dev)
    if not train_bn:
        call('dmy_bn_eval_coef', ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
             float(bn.eps), K, ptr(scale), ptr(shift), stream())
        return scale, shift, const_vec(K, 0.0, dev), const_vec(K, 1.0, dev)
    mean, invstd = f32(K, dev), f32(K, dev)
    P = call('dmy_bn_partial_rows', M)
    psum, psq = f32(P * K, dev), f32(P * K, dev)
    call('dmy_actbn_stats', dcode(z), ptr(z), K, spec.act, M, K, ptr(psum), ptr(psq), stream())
    psum, psq, P = _fold_partials(psum, psq, P, K, dev)
    _bn_finalize(psum, psq, P, K, M, bn, mean, invstd, scale, shift, sync)
    return scale, shift, mean, invstd


def _actbn_infer(x, g, wf, bias, spec, res, rps, y, yps):
    """inference of conv -> act -> eval BN (+ residual).  Depthwise 9x9: one launch (dmy_dwconv_fwd_actbn).  Dense: the
    conv with the activation in its epilogue, then one dmy_actbn_fwd for the affine map and the residual (folding that
    into the conv epilogue is the follow-up).  Any other depthwise size: the plain forward into z, then
    dmy_actbn_fwd with the activation, as in training."""
    scale, shift = eval_coef(spec, x.device)
    dt = dcode(x)
    if g.groups != 1 and g.k != 9:
        z = new_act(g.N, g.K, g.OH, g.OW, x)
        _launch_conv_fwd(x, g, wf, bias, z, g.K, None, None)
        call('dmy_actbn_fwd', dt, ptr(z), g.K, spec.act, ptr(scale), ptr(shift), ptr(res), rps, ptr(y), yps, g.M, g.K,
             stream())
        return y
    if g.groups != 1:
        _dw_check(dt, x, wf, y, g, g.xps, yps)
        KernelTimer.run('dwconv_fwd', g.flops(), 'dmy_dwconv_fwd_actbn', dt, ptr(x), ptr(wf), ptr(bias), ptr(y), *g.dw(),
                        yps, ptr(scale), ptr(shift), spec.act, ptr(res), rps, stream(), tag=g.tag(),
                        nbytes=x.element_size() * (g.N * g.H * g.W * g.C + g.k * g.k * g.C + g.M * g.C))
        return y
    t = new_act(g.N, g.K, g.OH, g.OW, x)
    _launch_conv_fwd(x, g, wf, bias, t, g.K, None, None, epi=(None, None, spec.act, None, 0))
    call('dmy_actbn_fwd', dt, ptr(t), g.K, ACT_NONE, ptr(scale), ptr(shift), ptr(res), rps, ptr(y), yps, g.M, g.K, stream())
    return y


class ConvActBNFn(torch.autograd.Function):
    """y = BN(act(conv(x) + bias)) (+ res).  Saves x, the prepped data-grad weight, z and the BN statistics; a = act(z)
    is recomputed in every pass.  The backward runs through the BN first and act' second, and the conv bias gets the
    column sums of dz (the apply pass writes their partial rows in the same launch)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, res, spec, xsink=None, rsink=None, grad_on=True, out=None):
        need_grad = grad_on and any(ctx.needs_input_grad[:6])  # see ConvBNActFn.forward
        bn = spec.bn
        train_bn = bn.training or not bn.track_running_stats
        infer = not need_grad and not train_bn
        sync = _bn_sync(bn, train_bn)  # raises under graph capture, ahead of this layer's first launch
        x, g, wf, wt, _ = _conv_operands(x, weight, spec, need_grad, infer)
        if g.K % VW[x.dtype] or g.s2d or g.Cp != g.C:
            raise NotImplementedError(f'conv -> act -> BN takes whole 16-byte vectors: output channels multiples of '
                                      f'{VW[x.dtype]} for {x.dtype}, got {g.K}')
        res, rps = vec_view(res) if res is not None else (None, 0)
        y, yps = out_or_new(out, (g.N, g.K, g.OH, g.OW), x)
        if not vec_ok(x.dtype, (), [yps], [y]):  # a view the vector kernels cannot address: a fresh output instead
            y, yps = new_act(g.N, g.K, g.OH, g.OW, x), g.K
        if infer:
            return _actbn_infer(x, g, wf, bias, spec, res, rps, y, yps)
        z = new_act(g.N, g.K, g.OH, g.OW, x)
        _launch_conv_fwd(x, g, wf, bias, z, g.K, None, None)
        scale, shift, mean, invstd = _actbn_stats(z, g, spec, bn, train_bn, sync)
        call('dmy_actbn_fwd', dcode(z), ptr(z), g.K, spec.act, ptr(scale), ptr(shift), ptr(res), rps, ptr(y), yps, g.M,
             g.K, stream())
        _save_ctx(ctx, (x, wt, z, scale, mean, invstd), g, spec, train_bn, None, weight, bias, gamma, beta,
                  res is not None, xsink, rsink, sync=sync)
        return y

    @staticmethod
    def backward(ctx, dy):
        g, spec = ctx.g, ctx.spec
        x, wt, z, scale, mean, invstd = ctx.saved_tensors
        dy, dps = vec_view(dy.to(z.dtype))
        K, M, dev, dt = g.K, g.M, dy.device, dcode(dy)
        dbias = dgamma = dbeta = None
        P = call('dmy_bn_partial_rows', M)
        if ctx.train_bn:
            pdb, pdg = f32(P * K, dev), f32(P * K, dev)
            call('dmy_actbn_bwd_reduce', dt, ptr(z), K, ptr(dy), dps, ptr(mean), ptr(invstd), spec.act, M, K, ptr(pdb),
                 ptr(pdg), stream())
            pdb, pdg, R = _fold_partials(pdb, pdg, P, K, dev)
            ca, cb, cc = f32(K, dev), f32(K, dev), f32(K, dev)
            dgamma, dbeta = _pgrad(ctx, 1, K, dev), _pgrad(ctx, 2, K, dev)
            _bn_bwd_finalize(pdb, pdg, R, K, M, spec.bn.weight, invstd, dgamma, dbeta, ca, cb, cc, ctx.sync)
        else:  # eval-mode BN is a fixed affine map
            ca, cb = scale, const_vec(K, 0.0, dev)
            cc = cb
        dz = new_act(g.N, K, g.OH, g.OW, z)
        pdz = f32(P * K, dev) if ctx.has_bias else None
        call('dmy_actbn_bwd_apply', dt, ptr(z), K, ptr(dy), dps, ptr(mean), ptr(invstd), spec.act, ptr(ca), ptr(cb),
             ptr(cc), ptr(dz), K, M, K, ptr(pdz), stream())
        if ctx.has_bias:
            dbias = _pgrad(ctx, 0, K, dev)
            call('dmy_reduce_rows', ptr(pdz), P, K, ptr(dbias), 0, stream())
        dx = _dgrad(ctx, dt, dz, K, wt, z) if ctx.needs_input_grad[0] else None
        dw = _conv_wgrad(ctx, dt, x, dz, K)[0] if ctx.needs_input_grad[1] else None
        dres = pass_or_self(ctx.rsink, dy) if ctx.has_res else None
        return dx, dw, dbias, dgamma, dbeta, dres, None, None, None, None, None


def conv_act_bn(x, weight, bias, bn, stride, pad, act, res=None, spec=None, xsink=None, rsink=None, out=None):
    """conv(+bias) -> act -> BatchNorm2d (+ res): conv_bn_act with the activation before the BN, as both halves of
    ConvMix (models/cspcm.py:28-37).  xsink / rsink / out as conv_bn_act.  The no-grad eval call is one launch for the
    depthwise 9x9 and two for a dense conv."""
    if spec is None:
        spec = _param_spec(weight._base if weight._base is not None else weight, stride, pad, act, bn)
    return ConvActBNFn.apply(x, weight, bias, bn.weight, bn.bias, res, spec, xsink, rsink, torch.is_grad_enabled(),
                             [out] if out is not None else None)
