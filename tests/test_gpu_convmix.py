"""GPU: ConvMix / CSPCM (models/cspcm.py:25-54) and a small model that contains them on the HIP path against the
reference fixtures (tests/golden/convmix.npz, cspcm.npz, cspcm_model.npz) and the plain-torch restatement
tests/convmix_ref.py.  Tolerances are tests/test_gpu_ghost.py's (modules) and tests/test_gpu_hor.py's (model)."""
import copy

import pytest
import torch

import convmix_ref
from golden_util import Fixture, load_sd
from oracle import nn as onn
from test_dm_ref import run_case
from test_gpu_ghost import _fwd_bwd, _close, _bf16_close, RTOL, ATOL, GRAD_TOL
from test_oracle_golden import check_module_case

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16, F32 = torch.bfloat16, torch.float32
BIAS = ('Resnet.0.bias', 'Conv_1x1.0.bias')


def _product():
    from dmayolo.models import common as P
    return {'ConvMix': P.ConvMix, 'CSPCM': P.CSPCM}


def _pair(name, args, seed=3):
    """(product module, restatement) with the same seeded parameters and BN statistics"""
    torch.manual_seed(seed)
    ref = onn.bn_defaults(convmix_ref.MODS[name](*args))
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


@pytest.mark.parametrize('name', ['convmix', 'cspcm'])
def test_module_vs_reference_golden_fp32(name):
    """train-mode forward and backward, the running statistics, and the eval-mode forward against the fixture"""
    fx = Fixture(name)
    res = run_case(fx, _product()[fx.meta['module']](*fx.meta['args']), 'cuda')
    check_module_case(fx, res, RTOL, ATOL, GRAD_TOL)
    gb = {k: v for k, v in res['gp'].items() if k.endswith(BIAS)}
    assert len(gb) == 2 and all(float(v.abs().max()) > 1e-3 for v in gb.values())  # true bias gradients, not zero
    for k, v in gb.items():
        want = fx.t(f'gp.{k}')
        torch.testing.assert_close(v, want, rtol=GRAD_TOL[0], atol=GRAD_TOL[1] * max(1, float(want.abs().max())))


@pytest.mark.parametrize('name,args,dtype', [('ConvMix', (32, 32), F32), ('ConvMix', (64, 64), BF16),
                                             ('CSPCM', (48, 64, 2), F32), ('CSPCM', (64, 128, 2), BF16)],
                         ids=['ConvMix-fp32', 'ConvMix-bf16', 'CSPCM-fp32', 'CSPCM-bf16'])
def test_module_vs_restatement(name, args, dtype):
    """an odd map with W no multiple of the strip (13 x 17), two chained ConvMix in CSPCM (the first writes its own
    tensor, the last into the concat buffer)"""
    prod, ref = _pair(name, args)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, args[0], 13, 17, generator=g)
    gup = torch.randn(2, args[1] if name == 'CSPCM' else args[0], 13, 17, generator=g)
    if dtype == BF16:
        x, gup = x.bfloat16().float(), gup.bfloat16().float()
    r = _fwd_bwd(ref, x, gup, 'cpu', F32)
    p = _fwd_bwd(prod, x, gup, 'cuda', dtype)
    (_close if dtype == F32 else _bf16_close)(p, r)
    for k in (k for k in r[2] if k.endswith(BIAS)):
        assert float(r[2][k].abs().max()) > 1e-3
        tol = (GRAD_TOL[0], GRAD_TOL[1]) if dtype == F32 else (6e-2, 6e-2)
        torch.testing.assert_close(p[2][k], r[2][k], rtol=tol[0], atol=tol[1] * max(1, float(r[2][k].abs().max())))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_eval_forward_no_grad_takes_the_inference_launches(dtype):
    """eval mode, parameters that require grad, under torch.no_grad(): one dmy_dwconv_fwd_actbn for the first stage, a
    conv with the GELU in its epilogue plus one dmy_actbn_fwd for the second -- no z, no statistics pass -- and the
    result equals the eval-mode forward taken with grad enabled (the training launches on the running statistics)"""
    from dmayolo import _lib
    prod, ref = _pair('CSPCM', (64, 64, 1))
    prod, ref = prod.cuda().eval(), ref.eval()
    assert all(p.requires_grad for p in prod.parameters())
    x = torch.randn(2, 64, 9, 11, generator=torch.Generator().manual_seed(6)).to(dtype).float()
    xi = x.cuda().to(dtype).contiguous(memory_format=CL)
    names = []
    _lib.TRACE[0] = lambda name, args: names.append(name)  # _lib.call's observer
    try:
        with torch.no_grad():
            y = prod(xi)
    finally:
        _lib.TRACE[0] = None
    assert names.count('dmy_dwconv_fwd_actbn') == 1 and names.count('dmy_actbn_fwd') == 1
    assert not any(n in names for n in ('dmy_actbn_stats', 'dmy_dwconv_fwd', 'dmy_bn_finalize')), names
    with torch.no_grad():
        yr = ref(x)
    yg = prod(xi.clone().requires_grad_(True)).detach()
    if dtype == F32:
        torch.testing.assert_close(y.float().cpu(), yr, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(yg.float().cpu(), yr, rtol=RTOL, atol=ATOL)
    else:
        from gpu_util import rel_err
        assert rel_err(y.float().cpu(), yr) < 3e-2 and rel_err(yg.float().cpu(), yr) < 3e-2


@pytest.mark.parametrize('k', [3, 7])
def test_conv_act_bn_eval_on_other_depthwise_sizes(k):
    """conv_act_bn on a depthwise conv the one-launch form does not take (dmy_dwconv_fwd_actbn is k = 9 only): the
    no-grad eval call runs the plain forward and dmy_actbn_fwd, and equals the eval forward taken with grad enabled bit
    for bit (the same two kernels) and torch's conv -> GELU -> BN in fp32"""
    import dmayolo.functional as Fn
    C = 16
    torch.manual_seed(k)
    conv = torch.nn.Conv2d(C, C, k, 1, k // 2, groups=C).cuda()
    bn = torch.nn.BatchNorm2d(C).cuda().eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5), bn.bias.normal_(0, 0.1), bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, C, 9, 11, device='cuda').contiguous(memory_format=CL)
    spec = Fn.spec_for(conv, 1, k // 2, Fn.ACT_GELU, bn)
    with torch.no_grad():
        y = Fn.conv_act_bn(x, conv.weight, conv.bias, bn, 1, k // 2, Fn.ACT_GELU, spec=spec)
        want = bn(torch.nn.functional.gelu(conv(x)))
    yg = Fn.conv_act_bn(x.clone().requires_grad_(True), conv.weight, conv.bias, bn, 1, k // 2, Fn.ACT_GELU, spec=spec)
    assert torch.equal(y, yg.detach())
    torch.testing.assert_close(y.cpu(), want.cpu(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ model

def _model(fx, dtype=F32):
    from dmayolo.models.yolo import Model
    m = convmix_ref.fixture_state(Model(fx.meta['yaml'], nc=fx.meta['nc'], act_dtype=dtype), fx)
    return m.cuda()


def test_model_train_eval_fp32():
    """tests/test_gpu_hor.py::test_model_train_eval_fp32's method and bounds on cspcm_model"""
    fx = Fixture('cspcm_model')
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
    assert sum(1 for k in gp if k.endswith(BIAS)) >= 6
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
    m.fuse()  # Conv layers fused, ConvMix's convs left alone: the same detections
    with torch.no_grad():
        zf, _ = m(x)
    torch.testing.assert_close(zf.cpu(), fx.t('eval_out'), rtol=1e-3, atol=2e-3)


def test_graphed_detector_and_tta_eval():
    """GraphedDetector's replay equals the eager eval forward bit for bit; augment=True runs"""
    from dmayolo.infer import GraphedDetector
    fx = Fixture('cspcm_model')
    m = _model(fx, BF16).eval()
    x = fx.t('in.0').cuda()
    with torch.no_grad():
        z = m(x)[0]
        gz = GraphedDetector(m)(x)[0]
        assert torch.equal(gz, z) and torch.equal(gz, m(x)[0])
        za, _ = m(x, augment=True)
    assert za.shape[0] == 2 and za.shape[2] == 15 and bool(torch.isfinite(za).all())
    ref = fx.t('eval_out')
    assert float((z.float().cpu() - ref).abs().max() / ref.abs().max()) < 2e-2


def test_trainer_step_deterministic_gradients():
    """one Trainer.step on cspcm_model under set_deterministic(True), twice from the same state: bit-identical gradients
    of every parameter of the CSPCM layers (the step is an accumulation step, so the gradients are still there)"""
    import dmayolo.functional as Fn
    from dmayolo.synthetic import images, targets, HYP_VISDRONE, scaled_hyp
    from dmayolo.trainer import Trainer
    fx = Fixture('cspcm_model')
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
            g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if k.startswith(('model.7.', 'model.12.'))}
            assert len(g) > 40 and all(v is not None for v in g.values())
            assert all(float(v.float().abs().max()) > 0 for k, v in g.items() if k.endswith(BIAS))
            grads.append(g)
        diff = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
        assert not diff, diff[:10]
    finally:
        Fn.set_deterministic(False)
