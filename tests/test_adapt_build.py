"""CPU: parse_model builds the adaptive-fusion YAMLs (AdaptConcat, Adapt_Add2, Adapt_Add3) with the reference's parameter
names, shapes and strides; AdaptADD is refused; the optimizer grouping puts Adapt_Add*.w into g1 (train.py:211-214).
No kernel runs here."""
import copy

import pytest
import torch

from golden_util import Fixture

# adaptconcat.yaml's layer list with every width halved (C3STR needs >= 64 channels: heads = c_ // 32)
ADAPTCONCAT_HALF = {
    'nc': 10, 'depth_multiple': 0.33, 'width_multiple': 1.0, 'anchors': 4,
    'backbone': [[-1, 1, 'Conv', [32, 6, 2, 2]], [-1, 1, 'Conv', [64, 3, 2]], [-1, 3, 'C3', [64]],
                 [-1, 1, 'Conv', [128, 3, 2]], [-1, 6, 'C3', [128]], [-1, 1, 'Conv', [256, 3, 2]], [-1, 9, 'C3', [256]],
                 [-1, 1, 'Conv', [512, 3, 2]], [-1, 3, 'C3', [512]], [-1, 1, 'SPPF', [512, 5]]],
    'head': [[-1, 1, 'Conv', [256, 1, 1]], [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']], [[-1, 6], 1, 'Concat', [1]],
             [-1, 3, 'C3', [256, False]], [-1, 1, 'Conv', [128, 1, 1]], [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],
             [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C3', [128, False]], [-1, 1, 'Conv', [64, 1, 1]],
             [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']], [[-1, 2], 1, 'AdaptConcat', [1, 64, 64]],
             [-1, 2, 'C3STR', [64, False]], [-1, 1, 'Conv', [64, 3, 2]], [[-1, 18, 4], 1, 'AdaptConcat', [1, 64, 64, 128]],
             [-1, 2, 'C3STR', [128, False]], [-1, 1, 'Conv', [128, 3, 2]],
             [[-1, 14, 6], 1, 'AdaptConcat', [1, 128, 128, 256]], [-1, 2, 'C3STR', [256, False]],
             [-1, 1, 'Conv', [256, 3, 2]], [[-1, 10], 1, 'AdaptConcat', [1, 256, 256]], [-1, 2, 'C3STR', [512, False]],
             [[21, 24, 27, 30], 1, 'Detect', ['nc', 'anchors']]],
}


def _build(yaml):
    from dmayolo.models.yolo import Model
    return Model(copy.deepcopy(yaml), nc=10)


def _check(m, meta):
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    want = meta['sd_shapes']
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    assert sd == want, [k for k in sd if sd[k] != want[k]]
    assert [k for k, _ in m.named_parameters()] == [k for k in want if k in dict(m.named_parameters())]
    assert [float(s) for s in m.stride] == meta['stride'] == [4.0, 8.0, 16.0, 32.0]
    assert [float(s) for s in m.model[-1].stride] == meta['stride']


@pytest.mark.parametrize('name', ['adapt_model_ca', 'adapt_model_spd6'])
def test_product_builds_fixture_yaml(name):
    fx = Fixture(name)
    m = _build(fx.meta['yaml'])
    _check(m, fx.meta)
    assert [str(s) for s in fx.z['pnames']] == [k for k, _ in m.named_parameters()]


def test_product_builds_adaptconcat_yaml_with_c3str():
    fx = Fixture('adapt_model_str')
    assert fx.meta['yaml'] == ADAPTCONCAT_HALF
    _check(_build(ADAPTCONCAT_HALF), fx.meta)


def test_module_keys_and_unused_weight_map2():
    from dmayolo.models.common import AdaptConcat, Adapt_Add2, Adapt_Add3
    for name, mod in (('adaptconcat_l2', AdaptConcat(2, 1, 24, 40)), ('adaptconcat_l3', AdaptConcat(3, 1, 32, 32, 64)),
                      ('adapt_add2', Adapt_Add2()), ('adapt_add3', Adapt_Add3(16, 16, 32))):
        want = Fixture(name).group('sd')
        sd = mod.state_dict()
        assert list(sd) == list(want) and all(sd[k].shape == want[k].shape for k in sd), name
    l2 = AdaptConcat(2, 1, 24, 40)
    assert tuple(l2.weight_map2.conv.weight.shape) == (16, 1, 1, 1)  # dim3 = 1, never used by a level-2 forward
    assert isinstance(l2.weight_map0.leaky, torch.nn.LeakyReLU) and l2.weight_map0.leaky.negative_slope == 0.1
    assert isinstance(l2.weight_map0.batch_norm, torch.nn.BatchNorm2d) and l2.weight_map0.conv.bias is None


def test_adaptadd_is_refused():
    y = copy.deepcopy(Fixture('adapt_model_ca').meta['yaml'])
    layers = y['backbone'] + y['head']
    i = next(i for i, l in enumerate(layers) if l[2] == 'AdaptConcat')
    layers[i][2] = 'AdaptADD'
    with pytest.raises(NotImplementedError, match='AdaptADD'):
        _build(y)


def test_leaky_slope():
    from dmayolo.models.common import act_code
    from dmayolo.functional import ACT_LEAKY
    assert ACT_LEAKY == 6 and act_code(torch.nn.LeakyReLU(0.1)) == ACT_LEAKY
    with pytest.raises(NotImplementedError, match='LeakyReLU'):
        act_code(torch.nn.LeakyReLU(0.01))


def test_optimizer_groups_put_adapt_add_w_in_g1():
    from dmayolo.models.common import Adapt_Add2, Adapt_Add3
    from dmayolo.optim import param_groups
    m = _build(Fixture('adapt_model_spd6').meta['yaml'])
    g0, g1, g2 = param_groups(m)
    ws = [v.w for v in m.modules() if isinstance(v, (Adapt_Add2, Adapt_Add3))]
    assert len(ws) == 6
    for w in ws:
        assert sum(p is w for p in g1) == 1 and not any(p is w for p in g0 + g2)
    conv = next(v.conv for v in m.modules() if isinstance(v, Adapt_Add3))
    assert any(p is conv.weight for p in g1) and any(p is conv.bias for p in g2)
    m = _build(Fixture('adapt_model_ca').meta['yaml'])
    g0, g1, g2 = param_groups(m)
    grouped = {id(p) for p in g0 + g1 + g2}
    assert all(id(p) in grouped for p in m.parameters())  # weight_levels, the level maps and the unused weight_map2
