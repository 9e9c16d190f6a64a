"""CPU: the SPD-mix fixtures (tools/gen_golden_dm.py, captured from the reference) against the plain-torch restatement
tests/dm_ref.py, at tests/test_adapt_ref.py's tolerance."""
import pytest
import torch

import dm_ref
from golden_util import Fixture, load_sd
from oracle import nn as onn
from test_oracle_golden import check_module_case

# torch.testing.assert_close's float32 defaults
RTOL, ATOL = 1.3e-6, 1e-5
MODULE_CASES = ['dmconv', 'dmmconv', 'dmmconv2']
MODEL_CASES = ['dm_model_cadmm', 'dm_model_cadmm2']


def run_case(fx, mod, device='cpu', dtype=torch.float32):
    """tests/adapt_ref.py::run_case for a module with one tensor input"""
    onn.bn_defaults(mod)
    load_sd(mod, fx.group('sd'))
    mod = mod.to(device)
    x = fx.seq('in')[0].to(device, dtype)
    if device != 'cpu':
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    mod.train()
    out = mod(x)
    gup = fx.seq('gup')[0].to(device, dtype)
    (out.float() * gup.float()).sum().backward()
    res = dict(out=[out.detach().float().cpu()], gin=[x.grad.float().cpu()],
               gp={k: p.grad.float().cpu() for k, p in mod.named_parameters() if p.grad is not None},
               buf={k: v.float().cpu().clone() for k, v in mod.state_dict().items() if 'running' in k})
    load_sd(mod, fx.group('sd'))
    mod.eval()
    with torch.no_grad():
        res['eout'] = [mod(x.detach()).float().cpu()]
    return res


@pytest.mark.parametrize('name', MODULE_CASES)
def test_restatement_reproduces_module(name):
    fx = Fixture(name)
    assert fx.meta['args'] == [16, 24] and tuple(fx.t('in.0').shape) == (2, 16, 12, 20)
    res = run_case(fx, dm_ref.MODS[fx.meta['module']](*fx.meta['args']))
    check_module_case(fx, res, RTOL, ATOL)
    assert tuple(res['out'][0].shape) == (2, {'dmconv': 96, 'dmmconv': 120, 'dmmconv2': 88}[name], 6, 10)


@pytest.mark.parametrize('name', MODEL_CASES)
def test_restatement_reproduces_model(name):
    fx = Fixture(name)
    assert fx.meta['nc'] == 10 and fx.meta['img'] == 64 and tuple(fx.t('in.0').shape) == (2, 3, 64, 64)
    m = dm_ref.fixture_state(onn.bn_defaults(dm_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
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
    assert any('.cv1.conv.weight' in k and k.startswith('model.1.') for k in gp)
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
