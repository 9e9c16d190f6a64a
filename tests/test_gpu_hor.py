"""GPU: csrc/hor.hip through the C ABI, and GnConv / HorBlock / C3HB and a small HorNet model on the HIP path against the
reference fixtures (tools/gen_golden_hor.py) and the plain-torch restatement tests/hor_ref.py.

Kernel bounds, against float64 torch on the stored inputs (which are exact in float64):
  gate, fp32: a * b * scale is two multiplies, each rounded once: 2 ulp of the result.  bf16: the fp32 product carries
      2^-23 relative, far below the one rounding to bf16 that follows, half an ulp of 8 significand bits: 2^-8 |ref|.
  layer scale forward, x + gamma * y: one multiply and one add (or one fma), each within 2^-24 of its own result, whose
      magnitudes |x| + |gamma y| bounds: 2^-23 (|x| + |gamma y|), plus 2^-8 |ref| for the bf16 store.
  dy = gamma * dout: one multiply, 1 ulp in fp32, 2^-8 |ref| in bf16.
  dgamma: the form tests/test_gpu_dw7.py uses for its reductions, 2^-18 sum |dout y|: a thread adds at most
      ceil(M / rows / RB) + RB + 1 <= 2^6 fp32 terms per channel for the shapes here, the rows are summed in double.
      The inputs are generated in the storage dtype, so their rounding adds nothing.
Every strided operand is a channel slice at a non-zero vector offset of a wider sentinel-filled buffer, the three
strides of a launch all different; every byte outside the target slices must come back unchanged.
Module tolerances are tests/test_gpu_ghost.py's, model bounds tests/test_gpu_dm.py's."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import hor_ref
from golden_util import Fixture
from gpu_util import rel_err
from oracle import nn as onn
from test_dm_ref import run_case
from test_gpu_ghost import RTOL, ATOL, GRAD_TOL, _bf16_close
from test_hor_ref import check_case

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
IDS = ['float32', 'bfloat16']
SENTINEL = 0x5A
CVS = [1, 3, 31]


def _vw(dtype):
    return 8 if dtype == BF16 else 4


def _wide(M, C, extra, off, dtype, gen=None):
    """-> (buffer [M, C + extra vectors] filled with the sentinel byte, its channel slice [off vectors : +C], pixel
    stride); the slice holds N(0, 1) values when gen is given"""
    vw = _vw(dtype)
    ps = C + extra * vw
    buf = torch.empty(M, ps, dtype=dtype, device='cuda')
    buf.view(torch.uint8).fill_(SENTINEL)
    sl = buf[:, off * vw:off * vw + C]
    if gen is not None:
        sl.copy_(torch.randn(M, C, generator=gen).to(dtype))
    return buf, sl, ps


def _untouched(buf, sl_cols, before=None):
    """every byte of buf outside the channel slice sl_cols = (c0, c1) still holds the sentinel (before: the whole
    buffer must equal this earlier copy: a read-only operand)"""
    if before is not None:
        return torch.equal(buf.view(torch.uint8), before.view(torch.uint8))
    c0, c1 = sl_cols
    raw = buf.view(torch.uint8).view(buf.shape[0], -1)
    es = buf.element_size()
    return bool((raw[:, :c0 * es] == SENTINEL).all()) and bool((raw[:, c1 * es:] == SENTINEL).all())


def _ulp(ref):
    """one fp32 unit in the last place of each float64 value"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref), e - 24)


def _check(name, got, ref, bound):
    worst = float(((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f'{name}: max err / bound {worst:.3g}')
    assert worst <= 1.0, (name, worst)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('M', [1, 70, 4099])
@pytest.mark.parametrize('cv', CVS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_gate_kernels(dtype, cv, M):
    from dmayolo._lib import call, stream
    vw, dt = _vw(dtype), int(dtype == BF16)
    C = cv * vw
    gen = torch.Generator().manual_seed(1000 * cv + M)
    scale = float(np.float32(0.7))
    abuf, a, aps = _wide(M, C, 2, 1, dtype, gen)
    bbuf, b, bps = _wide(M, C, 3, 2, dtype, gen)
    ybuf, y, yps = _wide(M, C, 5, 3, dtype)
    assert len({aps, bps, yps}) == 3
    a0, b0 = abuf.clone(), bbuf.clone()
    call('dmy_gate_fwd', dt, _p(a), aps, _p(b), bps, _p(y), yps, M, C, scale, stream())
    torch.cuda.synchronize()
    A, B = a.double().cpu(), b.double().cpu()
    ref = A * B * scale
    _check('gate fwd', y, ref, 2 * _ulp(ref) if dtype == F32 else 2.0 ** -8 * ref.abs())
    assert _untouched(ybuf, (3 * vw, 3 * vw + C)) and _untouched(abuf, None, a0) and _untouched(bbuf, None, b0)
    # backward: dy, da, db on three more strides
    gbuf, dy, dps = _wide(M, C, 4, 2, dtype, gen)
    dabuf, da, daps = _wide(M, C, 6, 4, dtype)
    dbbuf, db, dbps = _wide(M, C, 7, 1, dtype)
    assert len({dps, daps, dbps}) == 3
    g0 = gbuf.clone()
    call('dmy_gate_bwd', dt, _p(dy), dps, _p(a), aps, _p(b), bps, _p(da), daps, _p(db), dbps, M, C, scale, stream())
    torch.cuda.synchronize()
    G = dy.double().cpu()
    for name, got, ref in (('gate da', da, G * B * scale), ('gate db', db, G * A * scale)):
        _check(name, got, ref, 2 * _ulp(ref) if dtype == F32 else 2.0 ** -8 * ref.abs())
    assert _untouched(dabuf, (4 * vw, 4 * vw + C)) and _untouched(dbbuf, (vw, vw + C))
    assert _untouched(gbuf, None, g0) and _untouched(abuf, None, a0) and _untouched(bbuf, None, b0)


def test_gate_refuses_partial_vectors():
    from dmayolo._lib import lib, stream
    x = torch.zeros(4, 16, device='cuda')
    for C, ps, t in ((6, 16, x), (8, 10, x), (8, 16, x[:, 1:])):
        rc = lib.dmy_gate_fwd(0, _p(t), ps, _p(x), 16, _p(x), 16, 4, C, 1.0, stream())
        assert rc != 0, (C, ps)


@pytest.mark.parametrize('M', [70, 4099])
@pytest.mark.parametrize('cv', CVS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_layerscale_kernels(dtype, cv, M):
    from dmayolo._lib import call, stream
    vw, dt = _vw(dtype), int(dtype == BF16)
    C = cv * vw
    rows = call('dmy_layerscale_bwd_rows', M)
    assert rows >= 3 and M % rows
    gen = torch.Generator().manual_seed(2000 * cv + M)
    xbuf, x, xps = _wide(M, C, 2, 1, dtype, gen)
    obuf, o, ops = _wide(M, C, 5, 3, dtype)
    y = torch.randn(M, C, generator=gen).to(dtype).cuda()
    gamma = (torch.rand(C, generator=gen) + 0.5).cuda()
    x0 = xbuf.clone()
    call('dmy_layerscale_fwd', dt, _p(x), xps, _p(y), _p(gamma), _p(o), ops, M, C, stream())
    torch.cuda.synchronize()
    X, Y, Gm = x.double().cpu(), y.double().cpu(), gamma.double().cpu()
    ref = X + Gm * Y
    bound = 2.0 ** -23 * (X.abs() + (Gm * Y).abs()) + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0)
    _check('layerscale fwd', o, ref, bound)
    assert _untouched(obuf, (3 * vw, 3 * vw + C)) and _untouched(xbuf, None, x0)
    # backward: dout strided, dy dense inside a guard band of rows, the partial rows likewise
    gbuf, dout, dps = _wide(M, C, 4, 2, dtype, gen)
    g0 = gbuf.clone()
    outs = []
    for _ in range(2):
        dyb = torch.empty(M + 2, C, dtype=dtype, device='cuda')
        dyb.view(torch.uint8).fill_(SENTINEL)
        part = torch.full((rows + 2, C), float('nan'), device='cuda')
        call('dmy_layerscale_bwd', dt, _p(dout), dps, _p(y), _p(gamma), _p(dyb[1:]), M, C, _p(part[1:]), stream())
        dgamma = torch.empty(C, device='cuda')
        call('dmy_reduce_rows', _p(part[1:]), rows, C, _p(dgamma), 0, stream())
        torch.cuda.synchronize()
        assert bool((dyb[0].view(torch.uint8) == SENTINEL).all()) and bool((dyb[-1].view(torch.uint8) == SENTINEL).all())
        assert bool(torch.isnan(part[0]).all()) and bool(torch.isnan(part[-1]).all())
        assert bool(torch.isfinite(part[1:-1]).all())  # every row written
        outs.append((dyb[1:-1].clone(), dgamma.clone(), part[1:-1].clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))  # bit-identical run to run
    dy, dgamma, _ = outs[0]
    D = dout.double().cpu()
    ref = Gm * D
    _check('layerscale dy', dy, ref, _ulp(ref) if dtype == F32 else 2.0 ** -8 * ref.abs())
    _check('layerscale dgamma', dgamma, (D * Y).sum(0), 2.0 ** -18 * (D * Y).abs().sum(0))
    assert _untouched(gbuf, None, g0)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_layerscale_fn_sink_and_out_slice(dtype):
    """LayerScaleAddFn: dx is dout handed to the sink -- with a contribution already there the result is the sum of the
    two -- and `out` takes a concat-buffer slice"""
    import dmayolo.functional as Fn
    gen = torch.Generator().manual_seed(5)
    N, C, H, W = 2, 3 * _vw(dtype), 5, 7
    mk = lambda: torch.randn(N, C, H, W, generator=gen).to(dtype).cuda().contiguous(memory_format=CL)  # noqa: E731
    x, y, first, gup = mk().requires_grad_(True), mk().requires_grad_(True), mk(), mk()
    gamma = (torch.rand(C, generator=gen) + 0.5).cuda().requires_grad_(True)
    sink = Fn.GradSink(2)
    cat = Fn.concat_buffer(N, 2 * C, H, W, x)
    out = Fn.LayerScaleAddFn.apply(x, y, gamma, sink, [cat[:, C:]])
    assert out.data_ptr() == cat[:, C:].data_ptr()
    ref = x.detach().double() + gamma.detach().double().view(1, -1, 1, 1) * y.detach().double()
    assert rel_err(out.detach().float().cpu(), ref.float().cpu()) < (1e-6 if dtype == F32 else 4e-3)
    assert sink.passthrough(first.clone()) is None  # an earlier contribution (a clone: the sink adopts its buffer)
    out.backward(gup)
    want = (first.float() + gup.float()).to(dtype)  # one fp32 add, one rounding to storage
    assert torch.equal(x.grad, want)
    torch.testing.assert_close(y.grad.float(), (gamma.detach().view(1, -1, 1, 1) * gup.float()).to(dtype).float())
    dg = (gup.double() * y.detach().double()).sum((0, 2, 3))
    assert rel_err(gamma.grad.cpu(), dg.float().cpu()) < 1e-5


# ------------------------------------------------------------------ modules

def _product():
    from dmayolo.models import common as P
    return {'GnConv': P.GnConv, 'HorBlock': P.HorBlock, 'C3HB': P.C3HB}


@pytest.mark.parametrize('name', ['gnconv', 'gnconv_s2', 'horblock', 'c3hb'])
def test_module_vs_reference_golden_fp32(name):
    fx = Fixture(name)
    res = run_case(fx, _product()[fx.meta['module']](*fx.meta['args']), 'cuda')
    assert any(k.endswith('gamma1') for k in res['gp']) or name.startswith('gnconv')
    check_case(fx, res, RTOL, ATOL, GRAD_TOL)


def _seeded(cls, args, seed):
    """a module with fill_state_dict's parameters, gamma1 / gamma2 ~ U(0.5, 1.5) (the same for product and restatement)"""
    m = hor_ref.fill_state_dict(onn.bn_defaults(cls(*args)))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.rsplit('.', 1)[-1] in ('gamma1', 'gamma2'):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
    return m


def _train_pass(m, x, gup, dev, dtype=F32):
    m = m.to(dev).train()
    x = x.detach().clone().to(dev, dtype)
    if dev != 'cpu':
        x = x.contiguous(memory_format=CL)
    x.requires_grad_(True)
    out = m(x)
    (out.float() * gup.to(dev).float()).sum().backward()
    return (out.detach().float().cpu(), x.grad.float().cpu(),
            {k: p.grad.float().cpu() for k, p in m.named_parameters() if p.grad is not None})


@pytest.mark.parametrize('name,args,cin', [('GnConv', (128, 256, 3, 2), 128), ('C3HB', (256, 256, 1), 256)],
                         ids=['gnconv-s2', 'c3hb'])
def test_module_bf16_vs_restatement(name, args, cin):
    """the narrowest widths bf16 storage takes (GnConv / HorBlock 128 wide); test_gpu_ghost.py's _bf16_close bounds"""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, cin, 8, 10, generator=gen).bfloat16().float()
    ref = _seeded(hor_ref.MODS[name], args, 21)
    oshape = ref.train()(x).shape
    gup = torch.randn(oshape, generator=gen).bfloat16().float()
    ref.zero_grad()
    r = _train_pass(ref, x, gup, 'cpu')
    p = _train_pass(_seeded(_product()[name], args, 21), x, gup, 'cuda', BF16)
    assert set(p[2]) == set(r[2])
    _bf16_close(p, r)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_horblock128(dtype):
    """HorBlock(128) against the reference fixture: fp32 at the module tolerances, bf16 by _bf16_close against the
    restatement (which tests/test_hor_ref.py pins to the same fixture)"""
    from dmayolo.models import common as P
    fx = Fixture('horblock128')
    x, gup = fx.t('in.0'), fx.t('gup.0')
    p = _train_pass(hor_ref.fixture_state(P.HorBlock(128), fx), x, gup, 'cuda', dtype)
    if dtype == BF16:
        r = _train_pass(hor_ref.fixture_state(hor_ref.HorBlock(128), fx), x, gup, 'cpu')
        return _bf16_close(p, r)
    torch.testing.assert_close(p[0], fx.t('out.0'), rtol=RTOL, atol=ATOL)
    gin = fx.t('gin.0')
    torch.testing.assert_close(p[1], gin, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1.0, float(gin.abs().max())))
    for k, g in fx.group('gp').items():
        torch.testing.assert_close(p[2][k], g, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    got = torch.tensor([float(p[2][k].norm()) for k in names], dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=5e-3, atol=1e-5)


def test_horblock_without_layer_scale_bf16():
    """layer_scale_init_value = 0: gamma is None, the residuals ride on proj_out's / pwconv2's epilogue (res=)"""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 128, 8, 10, generator=gen).bfloat16().float()
    gup = torch.randn(2, 128, 8, 10, generator=gen).bfloat16().float()
    r = _train_pass(_seeded(hor_ref.HorBlock, (128, 0., 0), 22), x, gup, 'cpu')
    prod = _seeded(_product()['HorBlock'], (128, 0., 0), 22)
    assert prod.gamma1 is None and prod.gamma2 is None
    p = _train_pass(prod, x, gup, 'cuda', BF16)
    assert set(p[2]) == set(r[2]) and not any('gamma' in k for k in p[2])
    _bf16_close(p, r)


def test_launch_trace():
    """a train-mode GnConv step: five gate launches each way, no slice copy, no torch.split backward (the gradients of
    fused_x and dw_abc are each one buffer that the gates and the depthwise data-grad write their slices of)"""
    from test_gpu_dm import _trace
    m = _seeded(_product()['GnConv'], (128, 128), 23).cuda().train()
    x = torch.randn(2, 128, 8, 10, generator=torch.Generator().manual_seed(3)).bfloat16().cuda()
    x = x.contiguous(memory_format=CL).requires_grad_(True)
    y, fw = _trace(lambda: m(x))
    assert fw.get('dmy_gate_fwd') == 5 and 'dmy_slice_copy' not in fw and fw.get('dmy_dwconv_fwd') == 1, fw
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        _, bw = _trace(lambda: y.float().sum().backward())
    assert bw.get('dmy_gate_bwd') == 5 and 'dmy_slice_copy' not in bw and bw.get('dmy_dwconv_dgrad') == 1, bw
    ops = {e.key for e in prof.key_averages()}
    assert not {'aten::add', 'aten::cat', 'aten::slice_backward'} & ops, sorted(ops)
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())


# ------------------------------------------------------------------ model

def _model(fx, dtype=F32):
    from dmayolo.models.yolo import Model
    m = hor_ref.fixture_state(Model(fx.meta['yaml'], nc=fx.meta['nc'], act_dtype=dtype), fx)
    return m.cuda()


def test_model_train_eval_fp32():
    """tests/test_gpu_dm.py::test_model_train_eval_fp32's method and bounds"""
    fx = Fixture('hor_model')
    m = _model(fx)
    sd0 = copy.deepcopy(m.state_dict())
    x = fx.t('in.0').cuda()
    m.train()
    outs = m(x)
    sum((o.float() * g.cuda()).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.float().cpu(), b, rtol=1e-3, atol=1e-3)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert sum(1 for k in gp if k.endswith(('.gamma1', '.gamma2'))) >= 2
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad.cpu(), g, rtol=2e-3, atol=2e-3 * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    got = torch.tensor([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in names],
                       dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=5e-3, atol=1e-5)
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    torch.testing.assert_close(z.cpu(), fx.t('eval_out'), rtol=1e-3, atol=2e-3)


def test_model_bf16():
    """tests/test_gpu_dm.py::test_model_bf16's rule: train maps rel-L2 <= 1.5 x the 'bf16_sink' emulation's + 2e-3, the
    concatenated gp.* <= 1.5 x the emulation's + 1e-2, eval max error over max value < 2e-2.  The yardstick is the
    emulation of tests/hor_ref.py (its Stored leaves round what the HIP path stores), not the product"""
    from precision_emu import emulate
    fx = Fixture('hor_model')
    gups = [g.bfloat16().float() for g in fx.seq('gup')]
    emu = hor_ref.fixture_state(onn.bn_defaults(hor_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
    emu = emulate(emu, 'bf16_sink').train()
    eo = emu(fx.t('in.0').bfloat16().float())
    sum((o * g).sum() for o, g in zip(eo, gups)).backward()
    ks = sorted(fx.group('gp'))
    cat = lambda d: torch.cat([d[k].flatten() for k in ks])  # noqa: E731
    ref_gp = cat(fx.group('gp'))
    e_out = [rel_err(a.detach(), b) for a, b in zip(eo, fx.seq('out'))]
    e_gp = rel_err(cat({k: p.grad for k, p in emu.named_parameters() if p.grad is not None}), ref_gp)
    m = _model(fx, BF16)
    sd0 = copy.deepcopy(m.state_dict())
    x = fx.t('in.0').cuda()
    m.train()
    outs = m(x)
    sum((o.float() * g.cuda()).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    p_out = [rel_err(a.float().cpu(), b) for a, b in zip(outs, fx.seq('out'))]
    p_gp = rel_err(cat({k: p.grad.float().cpu() for k, p in m.named_parameters() if p.grad is not None}), ref_gp)
    print('hor_model bf16 train maps rel-L2 product', ['%.2e' % v for v in p_out], 'emulation', ['%.2e' % v for v in e_out])
    print('hor_model bf16 gp rel-L2 product %.2e emulation %.2e' % (p_gp, e_gp))
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    ref = fx.t('eval_out')
    e = float((z.float().cpu() - ref).abs().max() / ref.abs().max())
    print('hor_model bf16 eval max err / max %.2e' % e)
    for a, b in zip(p_out, e_out):
        assert a <= 1.5 * b + 2e-3, (p_out, e_out)
    assert p_gp <= 1.5 * e_gp + 1e-2, (p_gp, e_gp)
    assert e < 2e-2, e


def test_graphed_detector_and_tta_eval():
    """GraphedDetector's replay equals the eager eval forward bit for bit; augment=True runs"""
    from dmayolo.infer import GraphedDetector
    fx = Fixture('hor_model')
    m = _model(fx, BF16).eval()
    x = fx.t('in.0').cuda()
    with torch.no_grad():
        z = m(x)[0]
        gz = GraphedDetector(m)(x)[0]
        assert torch.equal(gz, z) and torch.equal(gz, m(x)[0])
        za, _ = m(x, augment=True)
    assert za.shape[0] == 2 and za.shape[2] == 15 and bool(torch.isfinite(za).all())


def test_trainer_step_deterministic_gradients():
    """one Trainer.step on hor_model under set_deterministic(True), twice from the same state: bit-identical gradients
    of every HorBlock parameter (gamma1 / gamma2 included: they get a gradient although no optimizer group holds
    them).  The step is an accumulation step, so the gradients are still there afterwards"""
    import dmayolo.functional as Fn
    from dmayolo.synthetic import images, targets, HYP_VISDRONE, scaled_hyp
    from dmayolo.trainer import Trainer
    fx = Fixture('hor_model')
    base = _model(fx, BF16).train()
    base.hyp = scaled_hyp(HYP_VISDRONE, 10, 64)
    x, t = images(16, 64, seed=1, device='cuda'), targets(16, 10, per_image=6, seed=1, device='cuda')
    Fn.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            m = copy.deepcopy(base)
            tr = Trainer(m, dict(m.hyp), 16, nb=100)
            tr.i = 500
            tr.last_opt_step = tr.ni  # no optimizer step (and no zero_grad) on this call
            loss, _ = tr.step(x, t)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss).all())
            g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if '.m.' in k or k.startswith('model.5.')}
            assert len(g) > 60 and all(v is not None for v in g.values())
            assert sum(1 for k in g if k.endswith(('gamma1', 'gamma2'))) == 6
            assert all(float(v.float().abs().max()) > 0 for k, v in g.items() if k.endswith(('gamma1', 'gamma2')))
            grads.append(g)
        diff = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
        assert not diff, diff[:10]
    finally:
        Fn.set_deterministic(False)
