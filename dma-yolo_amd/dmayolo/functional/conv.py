"""The conv engine: conv (+ BatchNorm) (+ activation) (+ residual) as one autograd Function over csrc/conv.hip,
conv_wgrad.hip, dwconv.hip, bwd1x1.hip and bn.hip.  Geometry, weight prep, the weight-gradient arena, the per-layer
specs with their inference caches, the launches, and the phases of ConvBNActFn."""
import os
import weakref
from collections import namedtuple

import torch
import torch.distributed as dist

from .._lib import call, ptr, stream, ACT_NONE
from ._base import DT, VW, const_vec, conv_out_hw, dcode, f32, new_act, out_view, pixel_stride, vec_view, \
    zero_padded_channels
from .fp8 import F8_DELAYED, F8Emit, _conv_fp8, fp8_eligible
from .sinks import pass_or_self, sink_result, sink_target
from .spd import _spd_shape
from .timer import KernelTimer


WGRAD_OIHW, WGRAD_ZEROED = 1, 2  # dmy_conv_wgrad_ex flags
DETERMINISTIC = [False]  # set_deterministic(): split-K weight-grads through a workspace, reduced in split order


def set_deterministic(on=True):
    """Run-to-run bit-identical training steps on the conv / loss path: weight-gradient split-K partials go to a
    workspace reduced in split order (dmy_conv_wgrad_det) instead of fp32 atomics.  The loss kernels are always
    deterministic.  Costs one workspace write + read per split-K weight-grad launch."""
    DETERMINISTIC[0] = bool(on)


class ConvGeom(namedtuple('ConvGeom', 'N C H W xps K k s p OH OW M Cg Hg Wg kg sg pg Cp s2d groups', defaults=(1,))):
    """Geometry of one conv layer call, built once in ConvBNActFn.forward.  N C H W xps K k s p OH OW (M = N * OH * OW
    output pixels) describe the layer as the model sees it (timer flops and tags, gradient shapes); Cg Hg Wg kg sg pg
    are what the kernels are launched with.  The two differ only for the stem forms: space-to-depth (s2d = Cs, the k6
    s2 p2 conv runs as k3 s1 p1 over Cs channels of the half-size image) and channel-padded (Cp = Cg > C, the
    zero-padded storage read as 16-byte vectors against zero weights).  Otherwise s2d = 0 and Cp = C.  groups is 1 for the
    dense kernels and C (== K) for a depthwise layer, which runs on the dwconv kernels (csrc/dwconv.hip)."""
    __slots__ = ()

    def launch(self):  # the geometry arguments shared by the forward / weight-grad kernels, up to the output size
        return self.N, self.Hg, self.Wg, self.Cg, self.xps, self.K, self.kg, self.kg, self.sg, self.pg, self.OH, self.OW

    def tag(self):
        return self.N, self.C, self.H, self.W, self.K, self.k, self.s

    def flops(self):
        return 2.0 * self.M * self.K * (self.C // self.groups) * self.k * self.k

    def dw(self):  # the geometry arguments of the depthwise kernels, up to the output size
        return self.N, self.H, self.W, self.C, self.xps, self.k, self.k, self.s, self.p, self.OH, self.OW


def _wgrad(dt, x, dz, dzps, dw, g, flags):
    """one weight-gradient launch over the launch geometry (atomic split-K, or the deterministic workspace form)"""
    kw = dict(tag=g.tag(), nbytes=x.element_size() * (g.N * g.Hg * g.Wg * g.Cg + g.M * g.K) +
              4 * g.K * g.Cg * g.kg * g.kg)
    if DETERMINISTIC[0]:
        ne = call('dmy_conv_wgrad_ws_elems', dt, ptr(x), ptr(dz), *g.launch(), dzps, flags)
        ws = f32(ne, dz.device) if ne else None
        KernelTimer.run('conv_wgrad', g.flops(), 'dmy_conv_wgrad_det', dt, ptr(x), ptr(dz), ptr(dw), *g.launch(), dzps,
                        flags, ptr(ws), ne, stream(), **kw)
    else:
        KernelTimer.run('conv_wgrad', g.flops(), 'dmy_conv_wgrad_ex', dt, ptr(x), ptr(dz), ptr(dw), *g.launch(), dzps,
                        flags, stream(), **kw)


class WgradArena:
    """Per-training-forward fp32 buffer holding every conv / linear weight gradient of a Model in
    torch OIHW order.  Model.forward clears it with ONE fill; each weight-grad launch then
    accumulates straight into its slice (no per-launch memset, no layout pass), and the slice is
    handed to autograd as the parameter's gradient.  A new buffer per forward, so the previous
    step's .grad views are never overwritten (gradient accumulation stays correct); a weight used
    twice in one forward gets a fresh tensor the second time."""
    current = None
    ALIGN = 64  # elements (256 B): slices stay 16-B aligned for the vectorised optimizer kernels

    def __init__(self, buf, offsets):
        self.buf, self.offsets, self.taken = buf, offsets, set()

    @classmethod
    def layout(cls, params):
        """data_ptr -> (offset, numel) for every fp32 parameter that requires a gradient (conv / linear weights,
        BN gamma / beta, conv biases: every tensor the conv backward produces comes from here, so the
        optimizer's pointer tables see the same gradient addresses every step); total size"""
        offs, n = {}, 0
        for q in params:
            if q.dim() >= 1 and q.dtype == torch.float32 and q.requires_grad:
                offs[q.data_ptr()] = (n, q.numel())
                n += -(-q.numel() // cls.ALIGN) * cls.ALIGN
        return offs, n

    def take(self, key, shape):
        o = self.offsets.get(key)
        numel = 1
        for d in shape:
            numel *= d
        if o is None or o[1] != numel or key in self.taken:
            return None
        self.taken.add(key)
        return self.buf[o[0]:o[0] + numel].view(shape)


# Bumped whenever our kernels write parameters or BN buffers through raw pointers (fused optimizers, EMA,
# train-mode BN running statistics): torch's _version does not see those writes, so the inference caches
# (prepped weights, eval BN coefficients) key on this as well.
PARAM_GEN = [0]


class WeightPrep:
    """Training forward: the activation-dtype copies of every conv weight of a Model (OHWI forward operand,
    IHWO data-grad operand) written by ONE dmy_conv_wprep_multi launch per forward instead of one
    dmy_conv_wprep per layer.  Buffer, operand views and the 40-byte device descriptor table are built once
    per model (host work per step: one launch).  Reusing the buffer is safe: its content is a pure function
    of the current weights, which change only at optimizer.step, between a backward and the next forward."""
    current = None
    ALIGN = 64  # elements: every operand 16-B aligned (v3 loaders)

    def __init__(self, weights, dtype, dev):
        import numpy as np
        sizes = [-(-w.numel() // self.ALIGN) * self.ALIGN for w in weights]
        self.buf = torch.empty(2 * sum(sizes), dtype=dtype, device=dev)
        self.map, recs, off = {}, [], 0
        for w, n in zip(weights, sizes):
            K, C, KH, KW = w.shape
            wf = self.buf[off:off + w.numel()].view(K, KH * KW * C)
            wt = self.buf[off + n:off + n + w.numel()].view(C, KH * KW * K)
            self.map[w.data_ptr()] = (wf, wt)
            recs.append((w.data_ptr(), wf.data_ptr(), wt.data_ptr(), K, C, KH, KW))
            off += 2 * n
        rec = np.dtype([('w', '<u8'), ('wf', '<u8'), ('wt', '<u8'), ('K', '<i4'), ('C', '<i4'), ('KH', '<i4'),
                        ('KW', '<i4')])
        self.table = torch.from_numpy(np.array(recs, dtype=rec).view(np.uint8)).to(dev)
        self.n, self.dtype = len(recs), dtype

    def launch(self):
        call('dmy_conv_wprep_multi', DT[self.dtype], ptr(self.table), self.n, stream())
        return self

    def get(self, weight, dtype):
        return self.map.get(weight.data_ptr()) if dtype == self.dtype else None


class ConvSpec:
    """Static description of one conv(+BN)(+act) layer; `bn` is the live nn.BatchNorm2d / nn.SyncBatchNorm (or None).
    wcache / ecache: inference-only caches of the prepped weight and the eval BN coefficients."""
    __slots__ = ('stride', 'pad', 'act', 'bn', 'wcache', 'ecache', 'fp8', 'f8cache', 'f8_emit', 'defer', 'groups',
                 '__weakref__')

    def __init__(self, stride, pad, act, bn=None):
        self.stride, self.pad, self.act, self.bn = int(stride), int(pad), int(act), bn
        self.wcache = self.ecache = self.f8cache = self.f8_emit = None
        self.fp8 = False
        self.defer = False  # deferred_affine(): the consumer applies this layer's BN (see SCGateFn)
        self.groups = 1  # nn.Conv2d.groups of the owning module (spec_for): > 1 selects the depthwise kernels


_SPECS = weakref.WeakKeyDictionary()


def spec_for(owner, stride, pad, act, bn):
    """The persistent ConvSpec of a conv module (keyed weakly on the module, so deepcopies such as the EMA
    model get their own)."""
    sp = _SPECS.get(owner)
    if sp is None or (sp.stride, sp.pad, sp.act) != (int(stride), int(pad), int(act)) or sp.bn is not bn:
        sp = _SPECS[owner] = ConvSpec(stride, pad, act, bn)
    sp.fp8 = bool(getattr(owner, 'dmy_fp8', False))
    sp.groups = int(getattr(owner, 'groups', 1))
    return sp


_PSPECS = {}  # id(weight parameter) -> (weakref, {(stride, pad, act, id(bn)): ConvSpec}); tensors cannot be
# WeakKeyDictionary keys (their == is elementwise)


def _param_spec(w, stride, pad, act, bn):
    k = id(w)
    ent = _PSPECS.get(k)
    if ent is None or ent[0]() is not w:
        ent = _PSPECS[k] = (weakref.ref(w, lambda _r, k=k: _PSPECS.pop(k, None)), {})
    key = (int(stride), int(pad), int(act), id(bn))
    sp = ent[1].get(key)
    if sp is None or sp.bn is not bn:
        sp = ent[1][key] = ConvSpec(stride, pad, act, bn)
    return sp


def drop_specs(model):
    """Forget every cached ConvSpec of `model`'s convs, with the inference caches hanging off them, and bump PARAM_GEN:
    for a change of module identity behind a conv (its BatchNorm replaced, utils.torch_utils.convert_sync_batchnorm).
    The next forward builds fresh specs around the live modules."""
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            _SPECS.pop(m, None)
            ent = _PSPECS.get(id(m.weight))
            if ent is not None and ent[0]() is m.weight:
                ent[1].clear()
    PARAM_GEN[0] += 1


# the two model-level fp8 entry points: they walk the spec registry above, the rest of the fp8 path is fp8.py

def set_fp8(model, on=True, min_k=3):
    """Config 5 (BASELINE configs[4]): run the forward of every eligible conv (input channels % 128 == 0, kernel
    >= min_k) on the fp8 e4m3 MFMA kernel; the backward stays bf16.  Default min_k = 3: a 1x1 layer is HBM /
    latency-bound, so its 2x MFMA rate does not pay for quantising its input (profiles/r02, c5 fp8 A/B).
    Returns the number of convs switched: those fp8_eligible's shape tests (C % 128, K % 8, K >= 32) admit; at run
    time the layer also needs bf16 activations and a quantised input under the descriptor range."""
    n = 0
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d) and m.groups == 1 and m.kernel_size[0] >= min_k \
                and fp8_eligible(m.in_channels, m.out_channels, torch.bfloat16, 0):
            m.dmy_fp8 = bool(on)
            n += 1
    PARAM_GEN[0] += 1  # drop cached inference weights / coefficients
    return n


def f8_saturation(model):
    """{module name: (saturated count, fraction)} of every delayed-scaling producer's last step"""
    out = {}
    for name, mod in model.named_modules():
        if not isinstance(mod, torch.nn.Conv2d):
            continue
        sps = [_SPECS[mod]] if mod in _SPECS else []  # module-held specs (common.conv_forward)
        ent = _PSPECS.get(id(mod.weight))
        if ent is not None and ent[0]() is mod.weight:
            sps += list(ent[1].values())
        for sp in sps:
            if isinstance(sp.f8_emit, F8Emit):
                out[name] = sp.f8_emit.saturated()
    return out


def prep_weight(w, dtype, need_t, Cp=None):
    K, C, KH, KW = w.shape
    Cp = Cp or C
    wc = w.detach().contiguous()
    wf = torch.empty((K, KH * KW * Cp), dtype=dtype, device=w.device)
    wt = torch.empty((C, KH * KW * K), dtype=dtype, device=w.device) if need_t else None
    call('dmy_conv_wprep', DT[dtype], ptr(wc), ptr(wf), ptr(wt), K, C, Cp, KH, KW, stream())
    return wf, wt


def _launch_conv_fwd(x, g, wf, bias, y, yps, psum, psq, epi=None, f8=None):
    """Launch over g's launch geometry; the timer's flops and tag are the layer's real ones (the stem forms differ).
    epi = (scale, shift, act, res, rps): fused inference epilogue (dmy_conv_fwd_act)
    f8 = (x8, amax, w8, wscale): run on the e4m3 kernel (dmy_conv_fwd_fp8, timer kind conv_fwd_f8)
    A depthwise layer (g.groups > 1) goes to _launch_dw_fwd with the same arguments."""
    if g.groups != 1:
        return _launch_dw_fwd(x, g, wf, bias, y, yps, psum, psq, epi)
    N, C, H, W, K, k, OH, OW = g.N, g.Cg, g.Hg, g.Wg, g.K, g.kg, g.OH, g.OW
    es, fl, geo = x.element_size(), g.flops(), g.launch()
    kw = dict(tag=g.tag(), nbytes=es * (N * H * W * C + K * C * k * k + N * OH * OW * K))
    sc, sh, act, res, rps = epi if epi is not None else (None, None, 0, None, 0)
    if f8 is not None:
        x8, amax, w8, ws = f8
        kw['nbytes'] = N * H * W * C + K * C * k * k + es * N * OH * OW * K
        KernelTimer.run('conv_fwd_f8', fl, 'dmy_conv_fwd_fp8', ptr(x8), ptr(w8), ptr(amax), ptr(ws), ptr(bias), ptr(y),
                        ptr(psum), ptr(psq), N, H, W, C, K, k, k, g.sg, g.pg, OH, OW, yps, ptr(sc), ptr(sh), act,
                        ptr(res), rps, stream(), **kw)
        return
    dt = dcode(x)
    ne = call('dmy_conv_fwd_splitk_elems', dt, ptr(x), ptr(wf), ptr(y), *geo, yps) if psum is None else 0
    if ne > 0:  # small M (batch-1 inference): split-K over the chip, reduced with the epilogue
        ws = f32(ne, x.device)
        KernelTimer.run('conv_fwd', fl, 'dmy_conv_fwd_act_ws', dt, ptr(x), ptr(wf), ptr(bias), ptr(y), *geo, yps,
                        ptr(sc), ptr(sh), act, ptr(res), rps, ptr(ws), ne, stream(), **kw)
    elif epi is None:
        KernelTimer.run('conv_fwd', fl, 'dmy_conv_fwd', dt, ptr(x), ptr(wf), ptr(bias), ptr(y), ptr(psum), ptr(psq),
                        *geo, yps, stream(), **kw)
    else:
        KernelTimer.run('conv_fwd', fl, 'dmy_conv_fwd_act', dt, ptr(x), ptr(wf), ptr(bias), ptr(y), *geo, yps, ptr(sc),
                        ptr(sh), act, ptr(res), rps, stream(), **kw)


def _dw_unsupported(groups, C, K, k, s, p):
    return NotImplementedError(f'grouped conv with groups != channels, or a depthwise geometry the gfx950 kernels do '
                               f'not take (dmy_dwconv_ok): groups={groups} C={C} K={K} k={k} s={s} p={p}')


def _dw_check(dt, a, w, b, g, aps, bps):
    """dmy_dwconv_ok for the launch about to be made: a / b are the tensors on the input / output side"""
    if not call('dmy_dwconv_ok', dt, ptr(a), ptr(w), ptr(b), g.N, g.H, g.W, g.C, g.K, g.groups, aps, g.k, g.k, g.s, g.p,
                g.OH, g.OW, bps):
        raise _dw_unsupported(g.groups, g.C, g.K, g.k, g.s, g.p)


def _launch_dw_fwd(x, g, w, bias, y, yps, psum, psq, epi):
    """depthwise forward: dmy_dwconv_fwd (training: z and the BN partial rows) or dmy_dwconv_fwd_act (inference
    epilogue).  w is the [k][k][C] filter operand (the IHWO copy of the (C, 1, k, k) weight)"""
    dt = dcode(x)
    _dw_check(dt, x, w, y, g, g.xps, yps)
    kw = dict(tag=g.tag(), nbytes=x.element_size() * (g.N * g.H * g.W * g.C + g.k * g.k * g.C + g.M * g.C))
    if epi is None:
        KernelTimer.run('dwconv_fwd', g.flops(), 'dmy_dwconv_fwd', dt, ptr(x), ptr(w), ptr(bias), ptr(y), ptr(psum),
                        ptr(psq), *g.dw(), yps, stream(), **kw)
    else:
        sc, sh, act, res, rps = epi
        KernelTimer.run('dwconv_fwd', g.flops(), 'dmy_dwconv_fwd_act', dt, ptr(x), ptr(w), ptr(bias), ptr(y), *g.dw(),
                        yps, ptr(sc), ptr(sh), act, ptr(res), rps, stream(), **kw)


def eval_coef(spec, dev):
    """eval-mode BN scale / shift from the running statistics (dmy_bn_eval_coef), cached on the spec until a
    parameter / buffer changes (torch _version, or PARAM_GEN for our in-place kernels)"""
    bn = spec.bn
    key = (PARAM_GEN[0],) + tuple((t.data_ptr(), t._version) if t is not None else None
                                  for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (float(bn.eps),)
    if spec.ecache is not None and spec.ecache[0] == key:
        return spec.ecache[1], spec.ecache[2]
    K = bn.running_mean.numel()
    scale, shift = f32(K, dev), f32(K, dev)
    call('dmy_bn_eval_coef', ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
         float(bn.eps), K, ptr(scale), ptr(shift), stream())
    spec.ecache = (key, scale, shift)
    return scale, shift


class BnLink:
    """A train-mode BN layer whose BN the consumer applies (SCConv's k3, applied by its gate: SCGateFn): the consumer's
    backward writes the layer's backward-reduce partials itself (dmy_scgate_bn_bwd), saving bn_bwd_reduce's pass over
    dy.  `ready` holds (the gradient buffer, its pixel stride, pdb, pdg, rows, its version); the producer's backward
    uses the partials only when the gradient it receives IS that buffer, unmodified, and falls back to
    dmy_bn_bwd_reduce otherwise.  (Round 2's data-grad-epilogue variant of the same partials, dmy_conv_dgrad_bn, measured
    slower end to end -- DMA-1536 140.8 -> 138.1 img/s, profiles/r02/ab_bnfuse.log -- and was removed in round 6.)"""
    __slots__ = ('scale', 'shift', 'mean', 'invstd', 'act', 'K', 'ready')

    def __init__(self, scale, shift, mean, invstd, act, K):
        self.scale, self.shift, self.mean, self.invstd, self.act, self.K = scale, shift, mean, invstd, act, K
        self.ready = None


# SCConv's k3 BatchNorm applied by its gate (SCGateFn, dmy_scgate_bn_*): DMY_DEFER_AFFINE=0 restores the separate
# bn_act_fwd / bn_bwd_reduce passes
DEFER_AFFINE = [os.environ.get('DMY_DEFER_AFFINE', '1') == '1']
# fused 1x1 backward (bwd1x1.hip): BN apply + data-grad + weight-grad of a train-mode 1x1 Conv-BN-act layer in one
# launch, dz never stored.  DMY_BWD1X1=0 restores the three-pass path (A/B, parity tests)
BWD1X1 = [os.environ.get('DMY_BWD1X1', '1') == '1']


def _fold_partials(a, b, P, K, dev):
    """Two-stage column reduction of two (P, K) partial arrays ahead of a one-block-per-channel finalize, -> (a', b',
    rows left).  Up to 4096 block rows: the finalize read them with a stride of K floats in 20 us per layer (97 layers
    per DMA-1536 step); the column sum reads them coalesced.  256 rows or fewer go to the finalize as they are."""
    if P <= 256:
        return a, b, P
    S = call('dmy_colsum2_rows', P)
    a2, b2 = f32(S * K, dev), f32(S * K, dev)
    call('dmy_colsum2', ptr(a), ptr(b), P, K, ptr(a2), ptr(b2), stream())
    return a2, b2, S


# ---- the phases of ConvBNActFn: forward in call order, then backward

def _conv_operands(x, weight, spec, need_grad, infer):
    """-> (x in its launch shape, ConvGeom, wf forward operand, wt data-grad operand or None, wkey) for the three input
    forms.  wkey is the weight's current value: inference reuses the operand (and the fp8 weight) cached under it."""
    s2d, cpad = getattr(x, '_dmy_s2d', 0), zero_padded_channels(x)
    wkey = (PARAM_GEN[0], weight.data_ptr(), weight._version, x.dtype, s2d)
    wf = spec.wcache[1] if infer and spec.wcache is not None and spec.wcache[0] == wkey else None
    K, C, k, _ = weight.shape
    s, p, wt = spec.stride, spec.pad, None
    if spec.groups != 1:
        return _dw_operands(x, weight, spec, need_grad, infer, wkey)
    x, xps = pixel_stride(x)
    if s2d:
        # stem over the space-to-depth image (image_s2d): the k6 s2 p2 conv runs as k3 s1 p1 over Cs channels
        assert C == s2d and k == 6 and s == 2 and p == 2, 's2d input feeds only the k6 s2 p2 stem'
        N, Cs, H2, W2 = x.shape
        g = ConvGeom(N, C, 2 * H2, 2 * W2, xps, K, k, s, p, H2, W2, N * H2 * W2, Cs, H2, W2, 3, 1, 1, C, Cs)
        if wf is None:
            wf = torch.empty((K, 9 * Cs), dtype=x.dtype, device=x.device)
            call('dmy_conv_wprep_s2d', DT[x.dtype], ptr(weight.detach().contiguous()), ptr(wf), K, C, Cs, stream())
            if infer:
                spec.wcache = (wkey, wf)
        return x, g, wf, wt, wkey
    N, Cx, H, W = x.shape
    assert Cx == C, (C, Cx)
    # stem: read the zero-padded storage as Cp channels (16-byte vectors) with zero weights
    Cp = cpad if (cpad and C % VW[x.dtype] and xps >= cpad) else C
    OH, OW = conv_out_hw(H, W, k, s, p)
    g = ConvGeom(N, C, H, W, xps, K, k, s, p, OH, OW, N * OH * OW, Cp, H, W, k, s, p, Cp, 0)
    pre = WeightPrep.current.get(weight, x.dtype) if WeightPrep.current is not None and Cp == C else None
    if wf is None and pre is not None:
        wf, wt = pre
    elif wf is None:
        wf, wt = prep_weight(weight, x.dtype, need_grad and Cp == C, Cp)
        if infer:
            spec.wcache = (wkey, wf)
    if Cp != C:
        x = x.as_strided((N, Cp, H, W), x.stride())
    return x, g, wf, wt, wkey


def _dw_operands(x, weight, spec, need_grad, infer, wkey):
    """_conv_operands for a depthwise layer (groups == C == K, weight (C, 1, k, k)): the filter operand is [k][k][C] in
    the activation dtype, which is exactly the IHWO copy the weight prep writes for K = C, C = 1, so forward and
    data-grad share it (returned as both wf and wt).  Any other grouping has no kernel."""
    K, one, k, k2 = weight.shape
    s, p, G = spec.stride, spec.pad, spec.groups
    if x.dim() != 4 or one != 1 or k != k2 or not (G == K == x.shape[1]) or getattr(x, '_dmy_s2d', 0):
        raise _dw_unsupported(G, x.shape[1] if x.dim() == 4 else -1, K, k, s, p)
    x, xps = pixel_stride(x)
    N, C, H, W = x.shape
    OH, OW = conv_out_hw(H, W, k, s, p)
    if OH < 1 or OW < 1 or C % VW[x.dtype] or p != k // 2 or (k, s) not in ((3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (9, 1)):
        raise _dw_unsupported(G, C, K, k, s, p)
    g = ConvGeom(N, C, H, W, xps, K, k, s, p, OH, OW, N * OH * OW, C, H, W, k, s, p, C, 0, G)
    w = spec.wcache[1] if infer and spec.wcache is not None and spec.wcache[0] == wkey else None
    pre = WeightPrep.current.get(weight, x.dtype) if WeightPrep.current is not None else None
    if w is None and pre is not None:
        w = pre[1]
    elif w is None:
        w = prep_weight(weight, x.dtype, True)[1]
        if infer:
            spec.wcache = (wkey, w)
    return x, g, w, w, wkey


def _conv_infer_spd(x, g, wf, bias, spec, out, yps, f8):
    """inference of an spd layer: the one-launch conv into a temporary, then dmy_space_to_depth into the destination
    (folding SM into the conv epilogue is the follow-up)"""
    t = _conv_infer(x, g, wf, bias, spec, None, 0, None, g.K, f8)
    y = out if out is not None else new_act(g.N, 4 * g.K, g.OH // 2, g.OW // 2, x)
    call('dmy_space_to_depth', dcode(x), ptr(t), g.K, ptr(y), yps, g.N, g.OH, g.OW, g.K, 0, stream())
    return y


def _conv_infer(x, g, wf, bias, spec, res, rps, out, yps, f8):
    """one fused launch: conv + eval-BN + act (+ residual)"""
    y = out if out is not None else new_act(g.N, g.K, g.OH, g.OW, x)
    scale, shift = eval_coef(spec, x.device) if spec.bn is not None else (None, None)
    epi = None if (scale is None and spec.act == ACT_NONE and res is None) else (scale, shift, spec.act, res, rps)
    _launch_conv_fwd(x, g, wf, bias, y, yps, None, None, epi=epi, f8=f8)
    return y


def _conv_bn_stats(x, g, wf, bias, z, bn, train_bn, f8, sync=None):
    """The conv launch into z and the BN coefficients -> (scale, shift, mean, invstd).  Train mode: the launch's
    epilogue writes per-row partial sums, folded and finalized (dmy_bn_finalize, which also updates the running
    statistics); eval-mode BN under autograd: scale / shift from the running statistics, mean / invstd unused."""
    K, M, dev = g.K, g.M, x.device
    scale, shift, mean, invstd = f32(K, dev), f32(K, dev), f32(K, dev), f32(K, dev)
    if not train_bn:
        _launch_conv_fwd(x, g, wf, bias, z, K, None, None, f8=f8)
        call('dmy_bn_eval_coef', ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
             float(bn.eps), K, ptr(scale), ptr(shift), stream())
        return scale, shift, mean, invstd
    # bf16 / fp32: rows for any route; the launch reports the rows its kernel wrote (halo / LANE: per wave).  A
    # depthwise launch writes exactly dmy_dwconv_fwd_rows rows
    dw = g.groups != 1
    P = call('dmy_dwconv_fwd_rows' if dw else 'dmy_conv_fwd_fp8_partial_rows' if f8 is not None else
             'dmy_conv_fwd_bound_rows', M, K)
    psum, psq = f32(P * K, dev), f32(P * K, dev)
    _launch_conv_fwd(x, g, wf, bias, z, K, psum, psq, f8=f8)
    if f8 is None and not dw:
        P = call('dmy_conv_fwd_last_rows')
    psum, psq, P = _fold_partials(psum, psq, P, K, dev)
    _bn_finalize(psum, psq, P, K, M, bn, mean, invstd, scale, shift, sync)
    return scale, shift, mean, invstd


def _bn_sync(bn, train_bn):
    """-> None for a BN layer that normalises with its own rank's statistics, else (process group, world size, rank):
    the layer exchanges its sums with the other ranks in both directions.  The conditions of
    torch.nn.SyncBatchNorm.forward: the module type, batch statistics in use, an initialised torch.distributed and a
    group of more than one rank.  A collective cannot be captured into a graph: such a layer raises under stream
    capture, and callers ask before the layer's first launch."""
    if not (train_bn and isinstance(bn, torch.nn.SyncBatchNorm)):
        return None
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group
    world = dist.get_world_size(group)
    if world <= 1:
        return None
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('SyncBatchNorm cannot run under graph capture: its cross-rank exchange of batch statistics '
                           'is a collective per layer (GraphedTrainStep / torch.cuda.graph); train a converted model '
                           'eagerly, or leave its BatchNorm2d layers unconverted')
    return group, world, dist.get_rank(group)


def _sync_slab(pa, pb, P, K, M, sync, dev):
    """The exchange of one synchronised layer, either direction: this rank's P partial rows packed into its slot of the
    fp64 slab [world][2K + 1] (dmy_bn_sync_pack zeros the other slots), then one all_reduce(SUM) ordered on the current
    stream -> the slab every rank holds alike.  M: this rank's pixel count (ranks may differ)."""
    group, world, rank = sync
    if M < 1:
        raise RuntimeError('SyncBatchNorm: a rank with no pixels in the batch is not supported')
    slab = torch.empty(world * (2 * K + 1), dtype=torch.float64, device=dev)
    call('dmy_bn_sync_pack', ptr(pa), ptr(pb), P, K, float(M), ptr(slab), world, rank, stream())
    dist.all_reduce(slab, op=dist.ReduceOp.SUM, group=group)
    return slab


def _bn_finalize(psum, psq, P, K, M, bn, mean, invstd, scale, shift, sync=None):
    """dmy_bn_finalize over P rows of per-channel partial sums of M values: writes mean / invstd / scale / shift and,
    for a training BN that tracks them, updates the running statistics in place.  sync (_bn_sync): the sums of every
    rank go into the statistics (dmy_bn_sync_finalize over the exchanged slab), so all ranks write the same bits."""
    upd = int(bn.training and bn.track_running_stats)
    if upd:
        PARAM_GEN[0] += 1  # running stats change behind torch's back: drop inference caches
    mom = bn.momentum if bn.momentum is not None else 0.0
    run = (ptr(bn.running_mean) if upd else None, ptr(bn.running_var) if upd else None,
           ptr(bn.num_batches_tracked) if upd else None, float(mom), float(bn.eps), upd,
           ptr(mean), ptr(invstd), ptr(scale), ptr(shift), stream())
    if sync is None:
        call('dmy_bn_finalize', ptr(psum), ptr(psq), P, K, float(M), ptr(bn.weight), ptr(bn.bias), *run)
    else:
        slab = _sync_slab(psum, psq, P, K, M, sync, mean.device)
        call('dmy_bn_sync_finalize', ptr(slab), sync[1], K, ptr(bn.weight), ptr(bn.bias), *run)


def _bn_bwd_finalize(pdb, pdg, P, K, M, gamma, invstd, dgamma, dbeta, ca, cb, cc, sync=None):
    """dmy_bn_bwd_finalize over P rows of (sum dy, sum dy * xhat) partials of M pixels: dgamma / dbeta and the apply
    coefficients.  sync (_bn_sync, as the forward decided): ca / cb / cc come from every rank's sums over the global
    pixel count, dgamma / dbeta stay this rank's own sums (torch's SyncBatchNorm rule: the DDP reducer averages them)."""
    if sync is None:
        call('dmy_bn_bwd_finalize', ptr(pdb), ptr(pdg), P, K, float(M), ptr(gamma), ptr(invstd), ptr(dgamma), ptr(dbeta),
             ptr(ca), ptr(cb), ptr(cc), stream())
    else:
        slab = _sync_slab(pdb, pdg, P, K, M, sync, ca.device)
        call('dmy_bn_sync_bwd_finalize', ptr(slab), sync[1], sync[2], K, ptr(gamma), ptr(invstd), ptr(dgamma),
             ptr(dbeta), ptr(ca), ptr(cb), ptr(cc), stream())


def _defer_affine(z, stats, act, K):
    """Deferred-affine exit: the consumer (SCGateFn) reads z and applies scale / shift itself, and hands this layer's
    backward the reduce partials through the BnLink returned here; z is valid only for that consumer."""
    # the link must NOT hold z here: z is this Function's OUTPUT, so ctx -> link -> z -> grad_fn -> ctx would
    # be a reference cycle through the C++ autograd node that Python's GC cannot break (round 4 leaked
    # every SCConv's z, ~4 GiB per DMA-1536 step).  The gate receives z as its own input.
    link = BnLink(*stats, act, K)
    z._dmy_affine, z._dmy_bnlink = stats, link
    return link


def _act_pass(g, z, scale, shift, spec, res, rps, out, yps, emit_ok, spd=False):
    """The activation pass y = act(z * scale + shift) (+ residual), into `out` when given.  emit_ok (a BN layer): when
    an fp8 consumer asked for it (spec.f8_emit), the pass also emits the e4m3 copy of y, attached as `_dmy_f8`.
    spd: the pass stores y in SM layout, (N, 4K, OH / 2, OW / 2) (dmy_bn_act_s2d_fwd; no residual, no e4m3 copy)."""
    K, M = g.K, g.M
    if spd:
        y = out if out is not None else new_act(g.N, 4 * K, g.OH // 2, g.OW // 2, z)
        call('dmy_bn_act_s2d_fwd', dcode(z), ptr(z), K, ptr(scale), ptr(shift), spec.act, ptr(y), yps, g.N, g.OH, g.OW,
             K, stream())
        return y
    y = out if out is not None else new_act(g.N, K, g.OH, g.OW, z)
    emit = spec.f8_emit if (emit_ok and F8_DELAYED[0] and z.dtype == torch.bfloat16 and K % 8 == 0 and yps % 8 == 0 and
                            (res is None or rps % 8 == 0)) else None
    if emit is not None and not torch.cuda.is_current_stream_capturing():
        e8 = emit.run(z, scale, shift, spec.act, res, rps, y, yps, M, K)
        if e8 is not None:
            y._dmy_f8 = e8
    else:
        call('dmy_bn_act_fwd', dcode(z), ptr(z), K, ptr(scale), ptr(shift), spec.act, ptr(res), rps, ptr(y), yps, M, K,
             stream())
    return y


def _save_ctx(ctx, saved, g, spec, train_bn, bnlink, weight, bias, gamma, beta, has_res, xsink, rsink, spd=False,
              sync=None):
    """everything ConvBNActFn.backward reads, set in this one place"""
    ctx.save_for_backward(*saved)
    ctx.g, ctx.spec, ctx.train_bn, ctx.bnlink, ctx.spd, ctx.sync = g, spec, train_bn, bnlink, spd, sync
    ctx.has_bias, ctx.has_res, ctx.xsink, ctx.rsink = bias is not None, has_res, xsink, rsink
    ctx.arena, ctx.wkey = WgradArena.current, weight.data_ptr()
    ctx.pkeys = tuple(t.data_ptr() if t is not None else None for t in (bias, gamma, beta))


def _pgrad(ctx, i, K, dev, zero=False):
    """the gradient tensor of parameter i of (bias, gamma, beta): its (zeroed) arena slice, else a fresh one"""
    key = ctx.pkeys[i]
    g = ctx.arena.take(key, (K,)) if (ctx.arena is not None and key is not None) else None
    return g if g is not None else torch.zeros(K, dtype=torch.float32, device=dev) if zero else f32(K, dev)


def _wgrad_target(ctx, shape, dev):
    """-> (dw, zeroed): the weight's slice of the step's zeroed arena, else a fresh uninitialised tensor"""
    dw = ctx.arena.take(ctx.wkey, shape) if ctx.arena is not None else None
    return (dw, True) if dw is not None else (torch.empty(shape, dtype=torch.float32, device=dev), False)


def _bn_bwd_coef(ctx, dt, dy, dps, z, stats, gamma):
    """-> (ca, cb, cc, dgamma, dbeta), the per-channel coefficients dmy_bn_bwd_apply and the fused 1x1 backward take.
    Train mode: the reduce partials come from the consumer through the BnLink or from dmy_bn_bwd_reduce, are folded,
    and dmy_bn_bwd_finalize writes the coefficients with dgamma / dbeta.  Eval-mode BN is a fixed affine map: ca =
    scale, cb = cc = 0, no parameter gradients.  stats = (scale, shift, mean, invstd)."""
    K, M, dev = ctx.g.K, ctx.g.M, dy.device
    ca, cb, cc = f32(K, dev), f32(K, dev), f32(K, dev)
    if not ctx.train_bn:
        ca.copy_(stats[0])
        cb.zero_()
        cc.zero_()
        return ca, cb, cc, None, None
    link, rd = ctx.bnlink, None
    if link is not None:
        rd, link.ready = link.ready, None
    if rd is not None and rd[0].data_ptr() == dy.data_ptr() and rd[1] == dps and rd[0]._version == rd[5]:
        _, _, pdb, pdg, P, _ = rd  # written by the consumer (data-grad epilogue / SCConv gate)
    elif ctx.spd:  # dy is in SM layout: the reduce reads it through the mapping, z in row order
        P = call('dmy_bn_bwd_reduce_s2d_rows', dt, M, K)
        pdb, pdg = f32(P * K, dev), f32(P * K, dev)
        call('dmy_bn_bwd_reduce_s2d', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), ctx.spec.act, ctx.g.N, ctx.g.OH,
             ctx.g.OW, K, ptr(pdb), ptr(pdg), stream())
    else:
        P = call('dmy_bn_reduce_rows', dt, ptr(z), K, ptr(dy), dps, M, K)
        pdb, pdg = f32(P * K, dev), f32(P * K, dev)
        call('dmy_bn_bwd_reduce', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), ctx.spec.act, M, K, ptr(pdb),
             ptr(pdg), stream())
    pdb, pdg, P = _fold_partials(pdb, pdg, P, K, dev)
    dgamma, dbeta = _pgrad(ctx, 1, K, dev), _pgrad(ctx, 2, K, dev)
    _bn_bwd_finalize(pdb, pdg, P, K, M, gamma, stats[3], dgamma, dbeta, ca, cb, cc, ctx.sync)
    return ca, cb, cc, dgamma, dbeta


def _bwd1x1(ctx, dy, dps, x, wt, z, stats, coef):
    """-> (dx, dw) when the fused kernel took the layer's apply + data-grad + weight-grad, else None.  Eligible: bf16
    storage, train-mode BN, 1x1 stride 1, both gradients wanted, a (K, C) pair the kernel
    is built for (dmy_conv1x1_bwd_bn_ok).  Deterministic mode: the weight-grad partials go through a workspace summed
    in block order instead of fp32 atomics.  stats = (scale, shift, mean, invstd), coef = (ca, cb, cc)."""
    g = ctx.g
    N, C, H, W, xps, K, M = g.N, g.C, g.H, g.W, g.xps, g.K, g.M
    if not (BWD1X1[0] and g.groups == 1 and ctx.train_bn and g.k == 1 and g.s == 1 and g.p == 0 and not g.s2d and g.Cp == C and
            dy.dtype == torch.bfloat16 and wt is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]):
        return None
    buf_probe = ctx.xsink.peek(N, C, H, W) if ctx.xsink is not None else None
    bps_probe = buf_probe[1] if buf_probe is not None else C
    if not call('dmy_conv1x1_bwd_bn_ok', M, K, C, dps, xps, bps_probe, ptr(dy), ptr(z), ptr(x),
                ptr(buf_probe[0]) if buf_probe is not None else ptr(z)):
        return None
    buf, bps, acc = sink_target(ctx.xsink, N, C, H, W, z)
    dw, zeroed = _wgrad_target(ctx, (K, C, 1, 1), dy.device)
    if not zeroed:  # the kernel accumulates
        dw.zero_()
    ne = call('dmy_conv1x1_bwd_bn_ws_elems', M, K, C) if DETERMINISTIC[0] else 0
    ws = f32(ne, dy.device) if ne else None
    KernelTimer.run('conv_bwd1x1', 4.0 * M * K * C, 'dmy_conv1x1_bwd_bn', ptr(dy), dps, ptr(z), ptr(x), xps, ptr(wt),
                    *map(ptr, stats), ctx.spec.act, *map(ptr, coef), ptr(buf), bps, acc, ptr(dw), ptr(ws), ne, M, K, C,
                    stream(), tag=g.tag(),
                    nbytes=z.element_size() * (2 * M * K + (2 + acc) * M * C + K * C) + 4 * K * C)
    return sink_result(ctx.xsink, buf), dw


def _dw_bias_in_wgrad(ctx):
    """a biased 7x7 depthwise layer without BN (get_dwconv, models/common.py:1361-1362): its weight-grad launch carries
    the bias gradient as one more partial row set (dmy_dwconv_wgrad_bias), so dz is not read a second time for it"""
    return ctx.g.groups != 1 and ctx.g.k == 7 and ctx.has_bias and ctx.spec.bn is None and ctx.needs_input_grad[1]


def _act_bias_bwd(ctx, dt, dy, dps, z, want_bias=True):
    """layer without BN -> (dz, its pixel stride, dbias): the activation's backward (dmy_bn_bwd_apply with the identity
    affine map; dz is dy itself behind ACT_NONE) and the bias gradient, the column sums of dz (None without a bias, or
    with want_bias off: the weight-grad launch produces it, see _dw_bias_in_wgrad)"""
    K, M, dev = ctx.g.K, ctx.g.M, dy.device
    dz, dzps, dbias = dy, dps, None
    if ctx.spd:  # the same pass also undoes the SM fold, so it runs behind ACT_NONE too
        dz, dzps = new_act(ctx.g.N, K, ctx.g.OH, ctx.g.OW, z), K
        zero, one = const_vec(K, 0.0, dev), const_vec(K, 1.0, dev)
        call('dmy_bn_bwd_apply_s2d', dt, ptr(z), K, ptr(dy), dps, ptr(one), ptr(zero), ptr(zero), ptr(one),
             ctx.spec.act, ptr(one), ptr(zero), ptr(zero), ptr(dz), K, ctx.g.N, ctx.g.OH, ctx.g.OW, K, stream())
    elif ctx.spec.act != ACT_NONE:
        dz, dzps = new_act(ctx.g.N, K, ctx.g.OH, ctx.g.OW, z), K
        zero, one = const_vec(K, 0.0, dev), const_vec(K, 1.0, dev)
        call('dmy_bn_bwd_apply', dt, ptr(z), K, ptr(dy), dps, ptr(one), ptr(zero), ptr(zero), ptr(one),
             ctx.spec.act, ptr(one), ptr(zero), ptr(zero), ptr(dz), K, M, K, stream())
    if ctx.has_bias and want_bias:
        P = call('dmy_bn_reduce_rows', dt, ptr(dz), dzps, None, 0, M, K)
        ps_, pq_ = f32(P * K, dev), f32(P * K, dev)
        call('dmy_bn_stats', dt, ptr(dz), dzps, M, K, ptr(ps_), ptr(pq_), stream())
        dbias = _pgrad(ctx, 0, K, dev)
        call('dmy_reduce_rows', ptr(ps_), P, K, ptr(dbias), 0, stream())
    return dz, dzps, dbias


def _dgrad(ctx, dt, dz, dzps, wt, z):
    """the data-grad launch, into the input's GradSink when it has one"""
    g = ctx.g
    N, C, H, W, K, k, M = g.N, g.C, g.H, g.W, g.K, g.k, g.M
    if g.Cp != C or g.s2d:
        raise NotImplementedError('input gradient of a channel-padded stem conv')
    buf, bps, acc = sink_target(ctx.xsink, N, C, H, W, z)
    if g.groups != 1:  # depthwise: a gather over dz, no atomics
        _dw_check(dt, buf, wt, dz, g, bps, dzps)
        KernelTimer.run('dwconv_dgrad', g.flops(), 'dmy_dwconv_dgrad', dt, ptr(dz), ptr(wt), ptr(buf), acc, N, H, W, C,
                        bps, k, k, g.s, g.p, g.OH, g.OW, dzps, stream(), tag=g.tag(),
                        nbytes=z.element_size() * (M * C + k * k * C + (1 + acc) * N * H * W * C))
        return sink_result(ctx.xsink, buf)
    KernelTimer.run('conv_dgrad', g.flops(), 'dmy_conv_dgrad', dt, ptr(dz), ptr(wt), ptr(buf), acc, N, H, W, C, bps, K,
                    k, k, g.s, g.p, g.OH, g.OW, dzps, stream(), tag=g.tag(),
                    nbytes=z.element_size() * (M * K + K * C * k * k + (1 + acc) * N * H * W * C))
    return sink_result(ctx.xsink, buf)


def _conv_wgrad(ctx, dt, x, dz, dzps, with_bias=False):
    """-> (dw, dbias): the weight gradient in torch OIHW order, in the weight's arena slice when it has one; dbias is
    None unless with_bias (_dw_bias_in_wgrad: the launch also sums dz per channel)"""
    g = ctx.g
    K, C, k, dev = g.K, g.C, g.k, dz.device
    if g.groups != 1:
        # depthwise: per-block partial rows [P][k * k * C], summed in row order into the (C, 1, k, k) gradient (no
        # atomics: bit-identical run to run with or without set_deterministic)
        dw, zeroed = _wgrad_target(ctx, (K, 1, k, k), dev)
        _dw_check(dt, x, dz, dz, g, g.xps, dzps)
        P = call('dmy_dwconv_wgrad_rows', g.M, C)
        # with_bias: rows of (k * k + 1) * C, the bias gradient's share follows the filter taps
        row, sfx = (k * k + int(with_bias)) * C, '_bias' if with_bias else ''
        part, dbias = f32(P * row, dev), _pgrad(ctx, 0, K, dev) if with_bias else None
        KernelTimer.run('dwconv_wgrad', g.flops(), 'dmy_dwconv_wgrad' + sfx, dt, ptr(x), ptr(dz), ptr(part), *g.dw(), dzps,
                        stream(), tag=g.tag(), nbytes=x.element_size() * (g.N * g.H * g.W * C + g.M * C) + 4 * row)
        call(f'dmy_dwconv_wgrad{sfx}_finalize', ptr(part), P, C, k, k, ptr(dw), int(zeroed),
             *((ptr(dbias), 0) if with_bias else ()), stream())
        return dw, dbias
    dw, zeroed = _wgrad_target(ctx, (K, C, k, k), dev)
    if g.s2d:
        dwo = f32(K * 9 * g.s2d, dev)
        _wgrad(dt, x, dz, dzps, dwo, g, 0)
        call('dmy_conv_wgrad_s2d_to_oihw', ptr(dwo), ptr(dw), K, C, g.s2d, stream())
    elif k == 1 and g.Cp == C:
        # 1x1: the GEMM view IS torch OIHW -> accumulate straight into the step's zeroed arena slice
        _wgrad(dt, x, dz, dzps, dw, g, WGRAD_OIHW | (WGRAD_ZEROED if zeroed else 0))
    else:
        # k > 1: OIHW-order atomics would scatter every tile row with stride k*k (measured 1.5x slower
        # weight-grad on yolov5s); accumulate in GEMM order, then one layout pass (drops stem padding)
        dwo = f32(K * g.Cp * k * k, dev)
        _wgrad(dt, x, dz, dzps, dwo, g, 0)
        call('dmy_conv_wgrad_to_oihw', ptr(dwo), ptr(dw), K, C, g.Cp, k, k, stream())
    return dw, None


class ConvBNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, res, spec, xsink=None, rsink=None, grad_on=True, out=None, spd=False):
        """out: None or [view] -- see out_view; ignored by a layer with no separate activation pass.  spd: the layer's
        output is SM(act(bn(conv(x)))), (N, 4K, OH / 2, OW / 2) -- see conv_bn_act"""
        f8in, prod = getattr(x, '_dmy_f8', None), getattr(x, '_dmy_prod', None)
        # ctx.needs_input_grad mirrors requires_grad even when the CALLER runs under torch.no_grad() (forward itself
        # always runs with grad disabled): `grad_on` is the caller's grad mode, so a no-grad call (detect / val with
        # parameters that require grad) takes the one-launch inference path
        need_grad = grad_on and any(ctx.needs_input_grad[:6])
        bn = spec.bn
        train_bn = bn is not None and (bn.training or not bn.track_running_stats)
        infer = not need_grad and not train_bn
        sync = _bn_sync(bn, train_bn)  # raises under graph capture, ahead of this layer's first launch
        x, g, wf, wt, wkey = _conv_operands(x, weight, spec, need_grad, infer)
        f8 = _conv_fp8(x, g, weight, spec, wkey, f8in, prod, infer)
        res, rps = pixel_stride(res) if res is not None else (None, 0)
        oshape = _spd_shape(g, x, res) if spd else (g.N, g.K, g.OH, g.OW)
        act_pass = spd or bn is not None or spec.act != ACT_NONE or res is not None
        out, yps = out_view(out and out[0], oshape, x) if act_pass else (None, None)
        yps = oshape[1] if out is None else yps
        if infer and spd:
            return _conv_infer_spd(x, g, wf, bias, spec, out, yps, f8)
        if infer:
            return _conv_infer(x, g, wf, bias, spec, res, rps, out, yps, f8)
        z, link = new_act(g.N, g.K, g.OH, g.OW, x), None
        if bn is None:
            _launch_conv_fwd(x, g, wf, bias, z, g.K, None, None, f8=f8)
            y = _act_pass(g, z, const_vec(g.K, 1.0, x.device), const_vec(g.K, 0.0, x.device), spec, res, rps, out, yps,
                          False, spd) if act_pass else z
            saved = (x, wt, z)
        else:
            stats = _conv_bn_stats(x, g, wf, bias, z, bn, train_bn, f8, sync)
            saved = (x, wt, z, *stats, bn.weight)
            if (spec.defer and DEFER_AFFINE[0] and train_bn and need_grad and x.dtype == torch.bfloat16 and
                    spec.act == ACT_NONE and res is None and out is None and g.K % 8 == 0 and f8 is None and
                    g.groups == 1 and not spd):
                y, link = z, _defer_affine(z, stats, spec.act, g.K)
            else:
                y = _act_pass(g, z, stats[0], stats[1], spec, res, rps, out, yps, True, spd)
                if x.dtype == torch.bfloat16 and g.K % 128 == 0 and train_bn and not spd:
                    y._dmy_prod = spec  # an fp8 consumer may ask this layer to emit its e4m3 copy (F8Emit)
        _save_ctx(ctx, saved, g, spec, train_bn, link, weight, bias, gamma, beta, res is not None, xsink, rsink, spd,
                  sync)
        return y

    @staticmethod
    def backward(ctx, dy):
        g, spec = ctx.g, ctx.spec
        x, wt, z, *bnt = ctx.saved_tensors
        dy, dps = (vec_view if ctx.spd else pixel_stride)(dy.to(z.dtype))  # the SM passes read dy as 16-byte vectors
        K, dev, dt = g.K, dy.device, dcode(dy)
        dbias = dgamma = dbeta = fused = None
        bias_in_wgrad = _dw_bias_in_wgrad(ctx)
        if spec.bn is not None:
            *stats, gamma = bnt
            *coef, dgamma, dbeta = _bn_bwd_coef(ctx, dt, dy, dps, z, stats, gamma)
            fused = None if ctx.spd else _bwd1x1(ctx, dy, dps, x, wt, z, stats, coef)
            if ctx.spd:
                dz, dzps = new_act(g.N, K, g.OH, g.OW, z), K
                call('dmy_bn_bwd_apply_s2d', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), spec.act, *map(ptr, coef),
                     ptr(dz), K, g.N, g.OH, g.OW, K, stream())
            elif fused is None:
                dz, dzps = new_act(g.N, K, g.OH, g.OW, z), K
                call('dmy_bn_bwd_apply', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), spec.act, *map(ptr, coef),
                     ptr(dz), K, g.M, K, stream())
            if ctx.has_bias and ctx.train_bn:
                dbias = _pgrad(ctx, 0, K, dev, zero=True)  # sum(dz) == 0 exactly behind train-mode BN
        else:
            dz, dzps, dbias = _act_bias_bwd(ctx, dt, dy, dps, z, want_bias=not bias_in_wgrad)
        if fused is not None:
            dx, dw = fused
        else:
            dx = _dgrad(ctx, dt, dz, dzps, wt, z) if ctx.needs_input_grad[0] else None
            dw = None
            if ctx.needs_input_grad[1]:
                dw, db = _conv_wgrad(ctx, dt, x, dz, dzps, bias_in_wgrad)
                dbias = db if bias_in_wgrad else dbias
        dres = pass_or_self(ctx.rsink, dy) if ctx.has_res else None
        return dx, dw, dbias, dgamma, dbeta, dres, None, None, None, None, None, None


def conv_bn_act(x, weight, bias, bn, stride, pad, act, res=None, spec=None, xsink=None, rsink=None, out=None,
                defer=False, spd=False):
    """xsink / rsink: GradSinks collecting the gradient of x / of the residual (see GradSink).  out: an NHWC view
    (a concat_buffer channel slice) the activation is written into instead of a fresh tensor, when the layer has a
    separate activation pass (BN and / or act / residual); the returned tensor is then that view.
    spd: the layer is followed by SM (models/common.py:1460-1467) and returns (N, 4K, OH / 2, OW / 2), `out` being a
    view of that shape.  Train mode folds SM into the activation pass and into the backward's reduce / apply passes
    (csrc/spd.hip); inference runs the one-launch conv into a temporary and dmy_space_to_depth into the destination.
    Such a layer takes no residual and never the deferred-affine exit, the fused 1x1 backward or the fp8 emit."""
    if spec is None:  # a persistent spec per weight PARAMETER (views made per call share their base), so the
        # inference caches (prepped weight, eval BN coefficients) hold across calls for the Detect / Swin / CBAM convs
        spec = _param_spec(weight._base if weight._base is not None else weight, stride, pad, act, bn)
    spec.defer = bool(defer)
    gamma = bn.weight if bn is not None else None
    beta = bn.bias if bn is not None else None
    return ConvBNActFn.apply(x, weight, bias, gamma, beta, res, spec, xsink, rsink, torch.is_grad_enabled(),
                             [out] if out is not None else None, bool(spd))
