"""GPU: the Ghost modules and a small yolov5s-ghost on the HIP path against the reference fixtures
(tests/golden/ghostbottleneck_s*.npz, ghost_v5s.npz) and the plain-torch restatement tests/ghost_ref.py.  Tolerances
are those of tests/test_gpu_modules.py (modules) and tests/test_gpu_model.py (model_v5s)."""
import copy

import pytest
import torch

import ghost_ref
from golden_util import Fixture, load_sd
from gpu_util import run_case, rel_err
from oracle import nn as onn
from test_oracle_golden import check_module_case

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5  # test_gpu_modules.py, fp32 storage
GRAD_TOL = (1e-3, 1e-4)
CL = torch.channels_last


def _product():
    from dmayolo.models import common as P
    return {'GhostBottleneck': P.GhostBottleneck, 'C3Ghost': P.C3Ghost, 'GhostConv': P.GhostConv, 'DWConv': P.DWConv}


def _pair(name, args, seed=3):
    """(product module, restatement) with the same seeded parameters and BN statistics"""
    torch.manual_seed(seed)
    ref = onn.bn_defaults(ghost_ref.MODS[name](*args))
    g = torch.Generator().manual_seed(seed)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    prod = onn.bn_defaults(_product()[name](*args))
    load_sd(prod, ref.state_dict())
    return prod, ref


def _fwd_bwd(mod, x, gup, device, dtype):
    mod = mod.to(device).train()
    xi = x.detach().clone().to(device, dtype)
    if device == 'cuda':
        xi = xi.contiguous(memory_format=CL)
    xi.requires_grad_(True)
    y = mod(xi)
    (y.float() * gup.to(device)).sum().backward()
    return (y.detach().float().cpu(), xi.grad.float().cpu(),
            {k: p.grad.float().cpu() for k, p in mod.named_parameters() if p.grad is not None})


def _close(res, ref):
    (y, dx, gp), (yr, dxr, gpr) = res, ref
    torch.testing.assert_close(y, yr, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dx, dxr, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1, float(dxr.abs().max())))
    assert set(gp) == set(gpr)
    for k, b in gpr.items():
        torch.testing.assert_close(gp[k], b, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1, float(b.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')


def _bf16_close(res, ref):
    """test_module_vs_oracle_bf16's bounds: output 3e-2, gradients 6e-2 (parameters as one concatenated vector)"""
    (y, dx, gp), (yr, dxr, gpr) = res, ref
    ks = sorted(gpr)
    e = (rel_err(y, yr), rel_err(dx, dxr),
         rel_err(torch.cat([gp[k].flatten() for k in ks]), torch.cat([gpr[k].flatten() for k in ks])))
    print('bf16 rel-L2 y / dx / params: %.2e %.2e %.2e' % e)
    assert e[0] < 3e-2 and e[1] < 6e-2 and e[2] < 6e-2, e


@pytest.mark.parametrize('name', ['ghostbottleneck_s1', 'ghostbottleneck_s2'])
def test_ghostbottleneck_vs_reference_golden_fp32(name):
    fx, res = run_case(name, _product(), 'cuda')
    check_module_case(fx, res, RTOL, ATOL, GRAD_TOL)
    _, ref = run_case(name, ghost_ref.MODS, 'cpu')  # and against the restatement
    for a, b in zip(res['out'] + res['gin'], ref['out'] + ref['gin']):
        torch.testing.assert_close(a, b, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1, float(b.abs().max())))


@pytest.mark.parametrize('name', ['ghostbottleneck_s1', 'ghostbottleneck_s2'])
def test_ghostbottleneck_bf16(name):
    fx, res = run_case(name, _product(), 'cuda', dtype=torch.bfloat16)
    _, ref = run_case(name, ghost_ref.MODS, 'cpu')
    _bf16_close((res['out'][0], res['gin'][0], res['gp']), (ref['out'][0], ref['gin'][0], ref['gp']))


@pytest.mark.parametrize('dtype,c', [(torch.float32, 32), (torch.bfloat16, 64)])
def test_c3ghost_vs_restatement(dtype, c):
    """C3Ghost(c, c, n=2).  fp32 at c = 32, whose narrowest depthwise layer has 4 channels (one fp32 vector); bf16
    storage needs whole 8-channel vectors (functional.VW), so it runs at c = 64 (narrowest layer 8 channels) and the
    c = 32 block is refused in bf16"""
    prod, ref = _pair('C3Ghost', (c, c, 2))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, c, 13, 17, generator=g)
    gup = torch.randn(2, c, 13, 17, generator=g)
    if dtype == torch.bfloat16:
        x, gup = x.bfloat16().float(), gup.bfloat16().float()
        small, _ = _pair('C3Ghost', (32, 32, 2))
        with pytest.raises(NotImplementedError, match='grouped conv with groups != channels'):
            small.cuda()(torch.zeros(1, 32, 8, 8, device='cuda', dtype=dtype).contiguous(memory_format=CL))
    r = _fwd_bwd(ref, x, gup, 'cpu', torch.float32)
    p = _fwd_bwd(prod, x, gup, 'cuda', dtype)
    (_close if dtype == torch.float32 else _bf16_close)(p, r)


def _model(fx, dtype=torch.float32):
    from dmayolo.models.yolo import Model
    m = Model(fx.meta['yaml'], nc=fx.meta['nc'], act_dtype=dtype)
    load_sd(m, fx.group('sd'))
    return m.cuda()


def test_ghost_model_train_eval_fp32():
    """test_gpu_model.py::test_model_train_eval_fp32's method and bounds on ghost_v5s"""
    fx = Fixture('ghost_v5s')
    m = _model(fx)
    x = fx.t('in.0').cuda()
    m.train()
    outs = m(x)
    sum((o.float() * g.cuda()).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.float().cpu(), b, rtol=1e-3, atol=1e-3)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert sum(1 for k in gp if params[k].dim() == 4 and params[k].shape[1] == 1 and params[k].shape[2] > 1) == 32
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad.cpu(), g, rtol=2e-3, atol=2e-3 * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    got = torch.tensor([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in names],
                       dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=5e-3, atol=1e-5)
    load_sd(m, fx.group('sd'))
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    torch.testing.assert_close(z.cpu(), fx.t('eval_out'), rtol=1e-3, atol=2e-3)


def test_ghost_model_bf16():
    """bf16 storage against the fp32 fixture.  Eval: test_gpu_model.py::test_model_bf16_close_to_fp32's measure and
    bound (max error over max value < 2e-2), the one bf16 check that file applies to model_v5s.  Train mode (batch
    statistics over as few as 8 values per channel at P5) has no bound there, so it is held to the error of the
    bf16-storage emulation of the restatement (tests/precision_emu.py 'bf16_sink', the method of
    test_gpu_bench_shape.py): rel-L2 of each map <= 1.5 x the emulation's + 2e-3, of the concatenated gp.* <= 1.5 x
    the emulation's + 1e-2.  The factor is that test's looser one, because the emulation rounds only leaf-module
    outputs: it misses the product's stored BN outputs of the linear (act=False) layers and the GhostBottleneck sums.
    At this fixture the emulation itself sits 4e-2 .. 9e-2 from the fp32 maps and about 1.1 from the fp32 gp.* (the
    gradient through 8-value batch statistics is ill-conditioned in bf16), so the gradient bound here is loose: the
    tight gradient checks are the fp32 model test above and the bf16 module tests."""
    from precision_emu import emulate
    fx = Fixture('ghost_v5s')
    gups = [g.bfloat16().float() for g in fx.seq('gup')]  # what autograd hands a bf16 output
    emu = onn.bn_defaults(ghost_ref.Model(fx.meta['yaml'], nc=fx.meta['nc']))
    load_sd(emu, fx.group('sd'))
    emu = emulate(emu, 'bf16_sink').train()
    eo = emu(fx.t('in.0').bfloat16().float())
    sum((o * g).sum() for o, g in zip(eo, gups)).backward()
    ks = sorted(fx.group('gp'))
    cat = lambda d: torch.cat([d[k].flatten() for k in ks])  # noqa: E731
    ref_gp = cat(fx.group('gp'))
    e_out = [rel_err(a.detach(), b) for a, b in zip(eo, fx.seq('out'))]
    e_gp = rel_err(cat({k: p.grad for k, p in emu.named_parameters()}), ref_gp)
    m = _model(fx, torch.bfloat16)
    x = fx.t('in.0').cuda()
    m.train()
    outs = m(x)
    sum((o.float() * g.cuda()).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    p_out = [rel_err(a.float().cpu(), b) for a, b in zip(outs, fx.seq('out'))]
    p_gp = rel_err(cat({k: p.grad.float().cpu() for k, p in m.named_parameters()}), ref_gp)
    print('bf16 train maps rel-L2 product', ['%.2e' % v for v in p_out], 'emulation', ['%.2e' % v for v in e_out])
    print('bf16 gp rel-L2 product %.2e emulation %.2e' % (p_gp, e_gp))
    for a, e in zip(p_out, e_out):
        assert a <= 1.5 * e + 2e-3, (p_out, e_out)
    assert p_gp <= 1.5 * e_gp + 1e-2, (p_gp, e_gp)
    load_sd(m, fx.group('sd'))
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    ref = fx.t('eval_out')
    e = float((z.cpu() - ref).abs().max() / ref.abs().max())
    print('bf16 eval max err / max %.2e' % e)
    assert e < 2e-2, e


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_ghost_model_one_launch_eval_fuse_and_graph(dtype):
    """eval: one launch per conv (no separate BN pass, depthwise layers on dmy_dwconv_fwd_act); fuse() changes the
    decoded output by no more than test_inference_epilogue_matches_unfused_and_tracks_updates allows for a fused
    model; GraphedDetector replays the eager forward bit for bit; augment=True runs"""
    from dmayolo import _lib
    from dmayolo.infer import GraphedDetector
    fx = Fixture('ghost_v5s')
    m = _model(fx, dtype).eval()
    x = fx.t('in.0').cuda()
    counts = {}

    def counting(name, args):  # _lib.call's observer: every launch, from whichever module
        counts[name] = counts.get(name, 0) + 1
    with torch.no_grad():
        ref, _ = m(x)
        _lib.TRACE[0] = counting
        try:
            z, _ = m(x)
        finally:
            _lib.TRACE[0] = None
        assert counts.get('dmy_bn_act_fwd', 0) == 0 and counts.get('dmy_dwconv_fwd', 0) == 0, counts
        assert counts.get('dmy_dwconv_fwd_act', 0) == 32, counts
        assert torch.equal(z, ref)
        if dtype == torch.bfloat16:
            gz = GraphedDetector(m)(x)[0]
            assert torch.equal(gz, m(x)[0])
        za, _ = m(x, augment=True)
        assert za.shape[0] == 2 and za.shape[2] == 15 and bool(torch.isfinite(za).all())
        m.fuse()
        c, _ = m(x)
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=5e-2, atol=6e-2)
    torch.testing.assert_close(c.float(), ref.float(), **tol)


def _trainer(base, bs):
    from dmayolo.trainer import Trainer
    m = copy.deepcopy(base)
    tr = Trainer(m, dict(m.hyp), bs, nb=100)
    tr.i = 500
    tr.last_opt_step = tr.ni  # no optimizer step (and no zero_grad) in this call: the gradients stay to be read
    return m, tr


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_ghost_trainer_step_and_determinism(dtype):
    """one Trainer.step on the fixture model with synthetic targets: finite loss, a gradient for every parameter,
    every depthwise weight gradient a view of the step's WgradArena buffer; and two seeded steps give bitwise-equal
    gradients under set_deterministic(True)"""
    import dmayolo.functional as Fn
    from dmayolo.synthetic import images, targets, HYP_VISDRONE, scaled_hyp
    fx = Fixture('ghost_v5s')
    base = _model(fx, dtype).train()
    base.hyp = scaled_hyp(HYP_VISDRONE, 10, 64)
    x, t = images(16, 64, seed=1, device='cuda'), targets(16, 10, per_image=6, seed=1, device='cuda')
    Fn.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            m, tr = _trainer(base, 16)
            loss, _ = tr.step(x, t)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss).all())
            missing = [k for k, p in m.named_parameters() if p.grad is None]
            assert not missing, missing
            assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
            offs, n = m._arena_layout[1], m._arena_layout[2]  # WgradArena.layout: data_ptr -> (offset, numel), size
            dws = [mod.weight for mod in m.modules() if isinstance(mod, torch.nn.Conv2d) and mod.groups > 1]
            assert len(dws) == 32
            for p in dws:  # the gradient lives in the step's arena buffer, at the weight's own offset
                st = p.grad.untyped_storage()
                assert st.nbytes() == 4 * n and p.grad.data_ptr() - st.data_ptr() == 4 * offs[p.data_ptr()][0]
                assert float(p.grad.abs().sum()) > 0
            grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
        diff = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
        assert not diff, diff[:10]
    finally:
        Fn.set_deterministic(False)
