"""CPU: parse_model builds the SPD-mix YAMLs (DMConv, DMMConv, DMMConv2) with the reference's parameter names, order,
shapes and strides; MP(k != 2) and odd map sizes are refused.  No kernel runs here."""
import copy

import pytest
import torch

from golden_util import Fixture


def _build(yaml):
    from dmayolo.models.yolo import Model
    return Model(copy.deepcopy(yaml), nc=10)


@pytest.mark.parametrize('name', ['dm_model_cadmm', 'dm_model_cadmm2', 'dm_model_dm'])
def test_product_builds_fixture_yaml(name):
    fx = Fixture(name)
    m, meta = _build(fx.meta['yaml']), fx.meta
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    want = meta['sd_shapes']
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    assert sd == want, [k for k in sd if sd[k] != want[k]]
    assert list(sd) == list(want)  # the reference's order
    assert [float(s) for s in m.stride] == meta['stride'] == [4.0, 8.0, 16.0, 32.0]
    assert [float(s) for s in m.model[-1].stride] == meta['stride']
    if fx.has('pnames'):
        assert [str(s) for s in fx.z['pnames']] == [k for k, _ in m.named_parameters()]
    kinds = {type(l).__name__ for l in m.model}
    assert {'dm_model_cadmm': 'DMMConv', 'dm_model_cadmm2': 'DMMConv2', 'dm_model_dm': 'DMConv'}[name] in kinds


def test_channel_rules_and_module_keys():
    """models/yolo.py:451-462: 5 * c2, c2 + 4 * c1, 4 * c2 output channels; no width multiple, no make_divisible"""
    from dmayolo.models import common as P
    from dmayolo.models.yolo import parse_model
    for name, want in (('DMMConv', 5 * 12), ('DMMConv2', 12 + 4 * 8), ('DMConv', 4 * 12)):
        d = {'nc': 10, 'anchors': 3, 'depth_multiple': 1.0, 'width_multiple': 0.5,
             'backbone': [[-1, 1, 'Conv', [16, 3, 1]], [-1, 1, name, [12]], [-1, 1, 'Conv', [16, 1, 1]]], 'head': []}
        layers, _ = parse_model(d, [3])
        assert layers[2].conv.in_channels == want, name
        assert isinstance(layers[1], getattr(P, name))
    for name, mod in (('dmconv', P.DMConv(16, 24)), ('dmmconv', P.DMMConv(16, 24)), ('dmmconv2', P.DMMConv2(16, 24))):
        want = Fixture(name).group('sd')
        sd = mod.state_dict()
        assert list(sd) == list(want) and all(sd[k].shape == want[k].shape for k in sd), name
    d = {'nc': 10, 'anchors': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0,
         'backbone': [[-1, 1, 'Conv', [16, 3, 1]], [-1, 1, 'SM', []], [-1, 1, 'MP', []], [-1, 1, 'Conv', [16, 1, 1]]],
         'head': []}
    layers, _ = parse_model(d, [3])
    assert isinstance(layers[1], P.SM) and isinstance(layers[2], P.MP) and layers[3].conv.in_channels == 64
    assert all(n in P.__all__ for n in ('SM', 'MP', 'DMConv', 'DMMConv', 'DMMConv2'))


def test_mp3_is_refused():
    from dmayolo.models.common import MP
    assert isinstance(MP().m, torch.nn.MaxPool2d) and isinstance(MP(2), torch.nn.Module)
    with pytest.raises(NotImplementedError, match='2 x 2'):
        MP(3)


@pytest.mark.parametrize('hw', [(7, 8), (8, 7), (1, 1)])
def test_odd_map_sizes_are_refused(hw):
    """the check runs before any kernel: a CPU tensor reaches it"""
    from dmayolo.models import common as P
    x = torch.zeros(1, 16, *hw)
    for mod in (P.DMConv(16, 24), P.DMMConv(16, 24), P.DMMConv2(16, 24), P.SM()):
        with pytest.raises(ValueError, match='even height and width'):
            mod(x)
