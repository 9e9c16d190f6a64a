"""GPU: DMConv / DMMConv / DMMConv2 and two small DM models on the HIP path against the reference fixtures
(tools/gen_golden_dm.py) and the plain-torch restatement tests/dm_ref.py.  Module tolerances are
tests/test_gpu_ghost.py's, model bounds those of its test_ghost_model_train_eval_fp32 / test_ghost_model_bf16."""
import copy

import pytest
import torch

import dm_ref
from golden_util import Fixture
from gpu_util import rel_err
from oracle import nn as onn
from test_dm_ref import run_case
from test_gpu_ghost import RTOL, ATOL, GRAD_TOL, _bf16_close
from test_oracle_golden import check_module_case

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32, BF16 = torch.float32, torch.bfloat16
MODULE_CASES = ['dmconv', 'dmmconv', 'dmmconv2']
MODEL_CASES = ['dm_model_cadmm', 'dm_model_cadmm2']


def _product():
    from dmayolo.models import common as P
    return {'DMConv': P.DMConv, 'DMMConv': P.DMMConv, 'DMMConv2': P.DMMConv2}


@pytest.mark.parametrize('name', MODULE_CASES)
def test_module_vs_reference_golden_fp32(name):
    fx = Fixture(name)
    res = run_case(fx, _product()[fx.meta['module']](*fx.meta['args']), 'cuda')
    check_module_case(fx, res, RTOL, ATOL, GRAD_TOL)


@pytest.mark.parametrize('name', MODULE_CASES)
def test_module_bf16_vs_restatement(name):
    """test_gpu_ghost.py::test_ghostbottleneck_bf16's method and bounds"""
    fx = Fixture(name)
    res = run_case(fx, _product()[fx.meta['module']](*fx.meta['args']), 'cuda', BF16)
    ref = run_case(fx, dm_ref.MODS[fx.meta['module']](*fx.meta['args']))
    _bf16_close((res['out'][0], res['gin'][0], res['gp']), (ref['out'][0], ref['gin'][0], ref['gp']))


def _model(fx, dtype=F32):
    from dmayolo.models.yolo import Model
    m = dm_ref.fixture_state(Model(fx.meta['yaml'], nc=fx.meta['nc'], act_dtype=dtype), fx)
    return m.cuda()


@pytest.mark.parametrize('name', MODEL_CASES)
def test_model_train_eval_fp32(name):
    """test_gpu_ghost.py::test_ghost_model_train_eval_fp32's method and bounds"""
    fx = Fixture(name)
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
    assert sum(1 for k in gp if '.cv1.conv.weight' in k or '.cv2.conv.weight' in k) >= 4
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


@pytest.mark.parametrize('name', MODEL_CASES)
def test_model_bf16(name):
    """test_gpu_ghost.py::test_ghost_model_bf16's rule: train maps rel-L2 <= 1.5 x the 'bf16_sink' emulation's + 2e-3,
    the concatenated gp.* <= 1.5 x the emulation's + 1e-2, eval max error over max value < 2e-2"""
    from precision_emu import emulate
    fx = Fixture(name)
    gups = [g.bfloat16().float() for g in fx.seq('gup')]
    emu = dm_ref.fixture_state(onn.bn_defaults(dm_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
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
    print(name, 'bf16 train maps rel-L2 product', ['%.2e' % v for v in p_out], 'emulation', ['%.2e' % v for v in e_out])
    print(name, 'bf16 gp rel-L2 product %.2e emulation %.2e' % (p_gp, e_gp))
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    ref = fx.t('eval_out')
    e = float((z.float().cpu() - ref).abs().max() / ref.abs().max())
    print(name, 'bf16 eval max err / max %.2e' % e)
    for a, b in zip(p_out, e_out):
        assert a <= 1.5 * b + 2e-3, (p_out, e_out)
    assert p_gp <= 1.5 * e_gp + 1e-2, (p_gp, e_gp)
    assert e < 2e-2, e


def test_graphed_detector_and_tta_eval():
    """GraphedDetector's replay equals the eager eval forward bit for bit; augment=True runs"""
    from dmayolo.infer import GraphedDetector
    fx = Fixture('dm_model_cadmm')
    m = _model(fx, BF16).eval()
    x = fx.t('in.0').cuda()
    with torch.no_grad():
        z = m(x)[0]
        gz = GraphedDetector(m)(x)[0]
        assert torch.equal(gz, z) and torch.equal(gz, m(x)[0])
        za, _ = m(x, augment=True)
    assert za.shape[0] == 2 and za.shape[2] == 15 and bool(torch.isfinite(za).all())


def test_trainer_two_steps_deterministic():
    """two Trainer.steps (optimizer steps included) on dm_model_cadmm, twice from the same state: bitwise-equal
    parameters and buffers under set_deterministic(True)"""
    import dmayolo.functional as Fn
    from dmayolo.synthetic import images, targets, HYP_VISDRONE, scaled_hyp
    from dmayolo.trainer import Trainer
    fx = Fixture('dm_model_cadmm')
    base = _model(fx, BF16).train()
    base.hyp = scaled_hyp(HYP_VISDRONE, 10, 64)
    x, t = images(16, 64, seed=1, device='cuda'), targets(16, 10, per_image=6, seed=1, device='cuda')
    Fn.set_deterministic(True)
    try:
        after = []
        for _ in range(2):
            m = copy.deepcopy(base)
            tr = Trainer(m, dict(m.hyp), 16, nb=100)
            tr.i = 500
            for _ in range(2):
                loss, _ = tr.step(x, t)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss).all())
            sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
            assert not torch.equal(sd['model.1.cv2.conv.weight'], base.state_dict()['model.1.cv2.conv.weight'])
            after.append(sd)
        diff = [k for k in after[0] if not torch.equal(after[0][k], after[1][k])]
        assert not diff, diff[:10]
    finally:
        Fn.set_deterministic(False)


def _trace(fn):
    from dmayolo import _lib
    counts = {}

    def counting(name, args):  # _lib.call's observer
        counts[name] = counts.get(name, 0) + 1
    _lib.TRACE[0] = counting
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.TRACE[0] = None
    return out, counts


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['float32', 'bfloat16'])
def test_launch_trace(dtype):
    """train-mode DMConv: SM rides on the activation pass and on the backward's BN passes (no dmy_space_to_depth, no
    plain bn_bwd_reduce / bn_bwd_apply).  DMMConv2: one dmy_spd_split_* per direction and no dmy_maxpool*.  Eval
    DMConv: the one-launch conv and one dmy_space_to_depth"""
    P = _product()
    x = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(0)).to(dtype).cuda()
    x = x.contiguous(memory_format=CL).requires_grad_(True)
    m = onn.bn_defaults(P['DMConv'](16, 24)).cuda().train()
    y, fw = _trace(lambda: m(x))
    assert tuple(y.shape) == (2, 96, 6, 10)
    assert fw.get('dmy_bn_act_s2d_fwd') == 1 and 'dmy_space_to_depth' not in fw and 'dmy_bn_act_fwd' not in fw, fw
    _, bw = _trace(lambda: y.float().sum().backward())
    assert bw.get('dmy_bn_bwd_reduce_s2d') == 1 and bw.get('dmy_bn_bwd_apply_s2d') == 1, bw
    assert not {'dmy_bn_bwd_reduce', 'dmy_bn_bwd_apply', 'dmy_space_to_depth', 'dmy_conv1x1_bwd_bn'} & set(bw), bw
    m.eval()
    with torch.no_grad():
        _, ev = _trace(lambda: m(x))
    assert ev.get('dmy_space_to_depth') == 1 and 'dmy_bn_act_fwd' not in ev and 'dmy_bn_act_s2d_fwd' not in ev, ev
    m2 = onn.bn_defaults(P['DMMConv2'](16, 24)).cuda().train()
    x.grad = None
    y2, fw2 = _trace(lambda: m2(x))
    _, bw2 = _trace(lambda: y2.float().sum().backward())
    both = {k: fw2.get(k, 0) + bw2.get(k, 0) for k in set(fw2) | set(bw2)}
    assert fw2.get('dmy_spd_split_fwd') == 1 and bw2.get('dmy_spd_split_bwd') == 1, (fw2, bw2)
    assert both['dmy_spd_split_fwd'] == 1 and both['dmy_spd_split_bwd'] == 1
    assert not [k for k in both if k.startswith('dmy_maxpool') or k in ('dmy_space_to_depth', 'dmy_slice_copy')], both
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())
