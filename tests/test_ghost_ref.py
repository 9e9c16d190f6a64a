"""CPU: the Ghost fixtures (tools/gen_golden_ghost.py, captured from the reference) against the plain-torch restatement
tests/ghost_ref.py, and the product Model's build of the Ghost YAML (no GPU: parameters and strides only)."""
import pytest
import torch

import ghost_ref
from golden_util import Fixture, load_sd
from oracle import nn as onn
from test_oracle_golden import run_module_case, check_module_case

# torch.testing.assert_close's float32 defaults
RTOL, ATOL = 1.3e-6, 1e-5


@pytest.mark.parametrize('name', ['ghostbottleneck_s1', 'ghostbottleneck_s2'])
def test_restatement_reproduces_ghostbottleneck(name):
    fx, res = run_module_case(name, build=lambda meta: ghost_ref.MODS[meta['module']](*meta['args']))
    assert fx.meta['args'][:2] == [32, 32] and tuple(fx.t('in.0').shape) == (2, 32, 13, 17)
    assert any(k.startswith('conv.2.') for k in fx.group('sd')) and ('conv.1.conv.weight' in fx.group('sd')) == \
        (fx.meta['args'][3] == 2)
    check_module_case(fx, res, RTOL, ATOL)


def test_restatement_reproduces_ghost_model():
    fx = Fixture('ghost_v5s')
    assert fx.meta['nc'] == 10 and fx.meta['img'] == 64 and tuple(fx.t('in.0').shape) == (2, 3, 64, 64)
    m = onn.bn_defaults(ghost_ref.Model(fx.meta['yaml'], nc=fx.meta['nc']))
    load_sd(m, fx.group('sd'))
    x = fx.t('in.0')
    m.train()
    outs = m(x)
    sum((o * g).sum() for o, g in zip(outs, fx.seq('gup'))).backward()
    for a, b in zip(outs, fx.seq('out')):
        torch.testing.assert_close(a.detach(), b)
    params = dict(m.named_parameters())
    gp = fx.group('gp')
    dws = [k for k, p in params.items() if p.dim() == 4 and p.shape[1] == 1 and p.shape[0] > 1 and p.shape[2] > 1]
    assert len(dws) == 32 and set(dws) <= set(gp) and min(params[k].shape[0] for k in dws) == 8
    for k, g in gp.items():
        torch.testing.assert_close(params[k].grad, g, rtol=RTOL, atol=ATOL * max(1.0, float(g.abs().max())),
                                   msg=lambda s, k=k: f'{k}: {s}')
    load_sd(m, fx.group('sd'))
    m.eval()
    with torch.no_grad():
        z, _ = m(x)
    torch.testing.assert_close(z, fx.t('eval_out'))


def test_product_model_builds_ghost_yaml():
    """Model(cfg) on the Ghost YAML: parse_model knows DWConv / GhostConv / GhostBottleneck / C3Ghost, the state_dict
    has the reference's keys and shapes, and the shape walk gives the strides"""
    from dmayolo.models.yolo import Model
    fx = Fixture('ghost_v5s')
    m = Model(fx.meta['yaml'], nc=10)
    sd, want = m.state_dict(), fx.group('sd')
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert [float(s) for s in m.stride] == [8.0, 16.0, 32.0]
    assert [float(s) for s in m.model[-1].stride] == [8.0, 16.0, 32.0]


def test_ghostbottleneck_keeps_reference_keys():
    from dmayolo.models.common import GhostBottleneck, C3Ghost, DWConv, Conv
    for s in (1, 2):
        fx = Fixture(f'ghostbottleneck_s{s}')
        sd = GhostBottleneck(32, 32, 3, s).state_dict()
        assert set(sd) == set(fx.group('sd'))
    assert isinstance(GhostBottleneck(32, 32).conv[1], torch.nn.Identity)
    assert isinstance(GhostBottleneck(32, 32).shortcut, torch.nn.Identity)
    assert issubclass(DWConv, Conv) and DWConv(16, 16, 3).conv.groups == 16
    assert set(C3Ghost(32, 32, 2).state_dict()) == set(ghost_ref.C3Ghost(32, 32, 2).state_dict())


def test_grouped_conv_that_is_not_depthwise_still_raises():
    from dmayolo.models.common import Conv
    m = Conv(16, 32, 3, g=2)
    with pytest.raises(NotImplementedError, match='grouped conv with groups != channels'):
        m(torch.zeros(1, 16, 8, 8).contiguous(memory_format=torch.channels_last))
