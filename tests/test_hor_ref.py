"""CPU: the HorNet fixtures (tools/gen_golden_hor.py, captured from the reference) against the plain-torch restatement
tests/hor_ref.py, at tests/test_dm_ref.py's tolerances."""
import pytest
import torch

import hor_ref
from golden_util import Fixture
from oracle import nn as onn
from test_dm_ref import RTOL, ATOL, run_case
from test_oracle_golden import check_module_case

MODULE_CASES = ['gnconv', 'gnconv_s2', 'horblock', 'c3hb']


@pytest.fixture(autouse=True)
def _capture_threads():
    """the fixtures were captured with 8 intra-op threads (tools/gen_golden.py); torch's CPU reductions split their
    range by thread count, and the bias gradients behind the five-deep gate chain differ by up to 1.6e-5 between 1 and
    8 threads, against the 1e-5 these tests allow.  Same partition as the capture, whatever the machine has"""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def check_case(fx, res, rtol, atol, grad_tol=None):
    """check_module_case for a fixture that keeps only the norm of some parameter gradients (gpnorm.<key>: c3hb's two
    pwconv weights, dropped for the committed-file limit)"""
    res = dict(res, gp=dict(res['gp']))
    gt = grad_tol or (rtol, atol)
    for k, n in fx.group('gpnorm').items():
        torch.testing.assert_close(res['gp'].pop(k).double().norm(), n.double(), rtol=gt[0], atol=gt[1],
                                   msg=lambda m, k=k: f'{k}: {m}')
    check_module_case(fx, res, rtol, atol, grad_tol)


@pytest.mark.parametrize('name', MODULE_CASES)
def test_restatement_reproduces_module(name):
    fx = Fixture(name)
    assert tuple(fx.t('in.0').shape) == (2, 64, 10, 12)
    for k, v in fx.group('sd').items():  # a branch scaled by 1e-6 would be invisible in the output
        if k.rsplit('.', 1)[-1] in ('gamma1', 'gamma2'):
            assert float(v.min()) >= 0.5 and float(v.max()) <= 1.5, k
    res = run_case(fx, hor_ref.MODS[fx.meta['module']](*fx.meta['args']))
    check_case(fx, res, RTOL, ATOL)
    want = {'gnconv': (2, 64, 10, 12), 'gnconv_s2': (2, 128, 5, 6), 'horblock': (2, 64, 10, 12), 'c3hb': (2, 128, 10, 12)}
    assert tuple(res['out'][0].shape) == want[name]


def test_restatement_reproduces_horblock128():
    fx = Fixture('horblock128')
    m = hor_ref.fixture_state(hor_ref.HorBlock(128), fx).train()
    x = fx.t('in.0').requires_grad_(True)
    out = m(x)
    (out * fx.t('gup.0')).sum().backward()
    torch.testing.assert_close(out.detach(), fx.t('out.0'), rtol=RTOL, atol=ATOL)
    gin = fx.t('gin.0')
    torch.testing.assert_close(x.grad, gin, rtol=RTOL, atol=ATOL * max(1.0, float(gin.abs().max())))
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert {'gamma1', 'gamma2', 'norm1.weight', 'gnconv.dwconv.weight', 'gnconv.pws.0.weight'} <= set(gp)
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad, g, rtol=RTOL, atol=ATOL * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    assert names == list(params)
    got = torch.tensor([float(params[k].grad.norm()) for k in names], dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=1e-4, atol=1e-6)


def test_restatement_reproduces_model():
    fx = Fixture('hor_model')
    assert fx.meta['nc'] == 10 and fx.meta['img'] == 64 and tuple(fx.t('in.0').shape) == (2, 3, 64, 64)
    m = hor_ref.fixture_state(onn.bn_defaults(hor_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == fx.meta['sd_shapes']
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    x = fx.t('in.0')
    m.train()
    outs = m(x)
    sum((o * g).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    assert len(outs) == 3
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.detach(), b)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert any(k.endswith('.gamma1') for k in gp) and any('.gnconv.pws.' in k for k in gp)
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad, g, rtol=RTOL, atol=ATOL * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    assert names == list(params)
    got = torch.tensor([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in names],
                       dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=1e-4, atol=1e-6)
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    torch.testing.assert_close(z, fx.t('eval_out'))
