"""CPU: the adaptive-fusion fixtures (tools/gen_golden_adapt.py, captured from the reference) against the plain-torch
restatement tests/adapt_ref.py, at tests/test_ghost_ref.py's tolerance."""
import pytest
import torch

import adapt_ref
from golden_util import Fixture
from oracle import nn as onn
from test_oracle_golden import check_module_case

# torch.testing.assert_close's float32 defaults
RTOL, ATOL = 1.3e-6, 1e-5
MODULE_CASES = ['adaptconcat_l2', 'adaptconcat_l3', 'adapt_add2', 'adapt_add3']
MODEL_CASES = ['adapt_model_ca', 'adapt_model_spd6']


@pytest.mark.parametrize('name', MODULE_CASES)
def test_restatement_reproduces_module(name):
    fx = Fixture(name)
    res = adapt_ref.run_case(fx, adapt_ref.MODS[fx.meta['module']](*fx.meta['args']))
    check_module_case(fx, res, RTOL, ATOL)
    if name == 'adaptconcat_l2':  # the level-2 module carries a weight_map2 that nothing uses
        assert 'weight_map2.conv.weight' in fx.group('sd') and 'weight_map2.conv.weight' not in fx.group('gp')
        torch.testing.assert_close(res['buf']['weight_map2.batch_norm.running_mean'],
                                   fx.group('sd')['weight_map2.batch_norm.running_mean'], rtol=0, atol=0)


@pytest.mark.parametrize('name', MODEL_CASES)
def test_restatement_reproduces_model(name):
    fx = Fixture(name)
    assert fx.meta['nc'] == 10 and fx.meta['img'] == 64 and tuple(fx.t('in.0').shape) == (2, 3, 64, 64)
    m = adapt_ref.fixture_state(onn.bn_defaults(adapt_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == fx.meta['sd_shapes']
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    x = fx.t('in.0')
    m.train()
    outs = m(x)
    sum((o * g).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    assert len(outs) == 4
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.detach(), b)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert any('.w' == k[-2:] or 'weight_levels' in k for k in gp)
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
