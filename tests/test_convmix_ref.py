"""CPU: the ConvMixer fixtures (tools/gen_golden_convmix.py, captured from the reference) against the plain-torch
restatement tests/convmix_ref.py, at tests/test_dm_ref.py's tolerances."""
import pytest
import torch
import torch.nn.functional as F

import convmix_ref
from golden_util import Fixture
from oracle import nn as onn
from test_dm_ref import RTOL, ATOL, run_case
from test_oracle_golden import check_module_case


@pytest.fixture(autouse=True)
def _capture_threads():
    """the fixtures were captured with 8 intra-op threads; same partition of torch's CPU reductions as the capture"""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def test_dw9_fixture_is_a_depthwise_9x9_same_conv():
    fx = Fixture('dw9')
    assert fx.meta['shapes'] == [[2, 8, 5, 7], [1, 24, 9, 13], [2, 16, 12, 18]]
    for i, (N, C, H, W) in enumerate(fx.meta['shapes']):
        x, w, b, dz = (fx.t(f'{i}.{k}') for k in ('x', 'w', 'b', 'dz'))
        assert tuple(x.shape) == (N, C, H, W) and tuple(w.shape) == (C, 1, 9, 9) and float(b.abs().min()) > 0
        x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
        y = F.conv2d(x, w, b, padding=4, groups=C)
        (y * dz).sum().backward()
        for got, k in ((y.detach(), 'y'), (x.grad, 'dx'), (w.grad, 'dw'), (b.grad, 'db')):
            want = fx.t(f'{i}.{k}')
            torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL * max(1.0, float(want.abs().max())),
                                       msg=lambda s, k=k: f'{i}.{k}: {s}')


@pytest.mark.parametrize('name', ['convmix', 'cspcm'])
def test_restatement_reproduces_module(name):
    fx = Fixture(name)
    assert tuple(fx.t('in.0').shape) == (2, 64, 10, 12)
    sd = fx.group('sd')
    for k, v in sd.items():  # non-trivial parameters: BN weight in [0.5, 1.5], conv biases as initialised (not zero)
        if k.endswith(('.2.weight', 'bn.weight')):
            assert float(v.min()) >= 0.5 and float(v.max()) <= 1.5, k
        if k.endswith('.0.bias'):
            assert float(v.abs().max()) > 0, k
    res = run_case(fx, convmix_ref.MODS[fx.meta['module']](*fx.meta['args']))
    check_module_case(fx, res, RTOL, ATOL)
    assert tuple(res['out'][0].shape) == (2, {'convmix': 64, 'cspcm': 128}[name], 10, 12)
    bias_grads = [k for k in res['gp'] if k.endswith(('Resnet.0.bias', 'Conv_1x1.0.bias'))]
    assert len(bias_grads) == 2 and all(float(res['gp'][k].abs().max()) > 1e-3 for k in bias_grads)


def test_restatement_reproduces_model():
    fx = Fixture('cspcm_model')
    assert fx.meta['nc'] == 10 and fx.meta['img'] == 64 and tuple(fx.t('in.0').shape) == (2, 3, 64, 64)
    m = convmix_ref.fixture_state(onn.bn_defaults(convmix_ref.Model(fx.meta['yaml'], nc=fx.meta['nc'])), fx)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == fx.meta['sd_shapes']
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    x = fx.t('in.0')
    m.train()
    outs = m(x)
    sum((o * g).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    assert len(outs) == 3 and tuple(outs[2].shape[2:4]) == (2, 2)  # the P5 map is under the 9x9 filter
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.detach(), b)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    assert any(k.endswith('Resnet.0.bias') for k in gp) and any(k.endswith('Conv_1x1.0.bias') for k in gp)
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad, g, rtol=RTOL, atol=ATOL * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    names = [str(s) for s in fx.z['pnames']]
    assert names == list(params)
    got = torch.tensor([float(params[k].grad.norm()) for k in names], dtype=torch.float64)
    torch.testing.assert_close(got, fx.t('gnorm'), rtol=1e-4, atol=1e-6)
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    torch.testing.assert_close(z, fx.t('eval_out'))
