"""CPU: parse_model builds YAMLs naming C3HB / HorBlock / GnConv with the reference's parameter names, order, shapes
and strides; the width / repeat rules, the stride walk, the optimizer grouping and the refusals.  No kernel runs here."""
import copy

import pytest
import torch

from golden_util import Fixture

CL = torch.channels_last


def _build(yaml):
    from dmayolo.models.yolo import Model
    return Model(copy.deepcopy(yaml), nc=10)


@pytest.mark.parametrize('name', ['hor_model', 'hor_model_fp32min'])
def test_product_builds_fixture_yaml(name):
    fx = Fixture(name)
    m, meta = _build(fx.meta['yaml']), fx.meta
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    want = meta['sd_shapes']
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    assert sd == want, [k for k in sd if sd[k] != want[k]]
    assert list(sd) == list(want)  # the reference's order
    assert [float(s) for s in m.stride] == meta['stride'] == [8.0, 16.0, 32.0]
    assert [float(s) for s in m.model[-1].stride] == meta['stride']
    if fx.has('pnames'):
        assert [str(s) for s in fx.z['pnames']] == [k for k, _ in m.named_parameters()]
    kinds = [type(l).__name__ for l in m.model]
    assert kinds.count('C3HB') == 2 and kinds.count('GnConv') == 1
    c_ = 128 if name == 'hor_model' else 64
    assert len(m.model[3].m) == 2 and len(m.model[6].m) == 1 and m.model[3].m[0].norm1.weight.numel() == c_
    assert m.model[5].proj_in.in_channels == c_ and m.model[5].proj_out.conv.stride == (2, 2)


def test_module_keys_match_the_reference():
    from dmayolo.models import common as P
    for name in ('gnconv', 'gnconv_s2', 'horblock', 'c3hb'):
        fx = Fixture(name)
        want = fx.group('sd')
        sd = getattr(P, fx.meta['module'])(*fx.meta['args']).state_dict()
        assert list(sd) == list(want) and all(sd[k].shape == want[k].shape for k in sd), name
    assert all(n in P.__all__ for n in ('LayerNorm', 'GnConv', 'HorBlock', 'C3HB'))
    ln = P.LayerNorm(16, eps=1e-5, data_format='channels_first')
    assert list(ln.state_dict()) == ['weight', 'bias'] and ln.eps == 1e-5 and ln.normalized_shape == (16,)
    g = P.GnConv(64, 64)
    assert g.dims == [4, 8, 16, 32, 64] and g.dwconv.groups == 124 and g.dwconv.bias is not None and g.scale == 1.0


def test_parse_model_width_and_repeat_rules():
    """models/yolo.py:388, 399: the three names are width-scaled, C3HB takes the repeat count as its n"""
    from dmayolo.models import common as P
    from dmayolo.models.yolo import parse_model
    d = {'nc': 10, 'anchors': 3, 'depth_multiple': 0.33, 'width_multiple': 0.5,
         'backbone': [[-1, 1, 'Conv', [128, 3, 1]], [-1, 3, 'C3HB', [256, False]], [-1, 1, 'GnConv', [256, 3, 2]]],
         'head': []}
    layers, _ = parse_model(d, [3])
    assert type(layers[1]) is P.C3HB and len(layers[1].m) == 1 and isinstance(layers[1].m[0], P.HorBlock)
    assert layers[1].cv1.conv.in_channels == 64 and layers[1].cv3.conv.out_channels == 128
    assert layers[1].m[0].gamma1.numel() == 64
    assert type(layers[2]) is P.GnConv and layers[2].proj_in.in_channels == 128
    assert layers[2].proj_out.conv.out_channels == 128 and layers[2].proj_out.conv.kernel_size == (3, 3)
    # a YAML-level HorBlock [c2] is HorBlock(dim=c1, drop_path=c2) under the width rule, in the reference too
    d['backbone'][2] = [-1, 1, 'HorBlock', [128]]
    with pytest.raises(NotImplementedError, match='drop_path'):
        parse_model(d, [3])


def test_gnconv_halves_the_stride_walk():
    d = {'nc': 10, 'anchors': [[10, 13, 16, 30, 33, 23]], 'depth_multiple': 1.0, 'width_multiple': 1.0,
         'backbone': [[-1, 1, 'Conv', [64, 6, 2, 2]], [-1, 1, 'GnConv', [128, 3, 2]], [-1, 1, 'C3HB', [128]]],
         'head': [[[2], 1, 'Detect', ['nc', 'anchors']]]}
    m = _build(d)
    assert [float(s) for s in m.stride] == [4.0]


def test_param_groups_placement():
    """train.py:197-214 looks at .weight, .bias and .w only: gamma1 / gamma2 land in no group (and still train's
    backward gives them a gradient -- tests/test_gpu_hor.py)"""
    from dmayolo.optim import param_groups
    m = _build(Fixture('hor_model').meta['yaml'])
    g0, g1, g2 = param_groups(m)
    ids = [{id(p) for p in g} for g in (g0, g1, g2)]
    where = {k: [i for i, s in enumerate(ids) if id(p) in s] for k, p in m.named_parameters()}
    blk = 'model.3.m.0.'
    for k in ('norm1.weight', 'norm2.weight', 'gnconv.proj_in.weight', 'gnconv.dwconv.weight', 'gnconv.pws.0.weight',
              'gnconv.proj_out.conv.weight', 'pwconv1.weight', 'pwconv2.weight'):
        assert where[blk + k] == [1], (k, where[blk + k])
    for k in ('norm1.bias', 'norm2.bias', 'gnconv.proj_in.bias', 'gnconv.dwconv.bias', 'gnconv.pws.0.bias',
              'gnconv.pws.3.bias', 'pwconv1.bias', 'pwconv2.bias'):
        assert where[blk + k] == [2], (k, where[blk + k])
    assert where[blk + 'gnconv.proj_out.bn.weight'] == [0] and where[blk + 'gnconv.proj_out.bn.bias'] == [2]
    gammas = [k for k in where if k.rsplit('.', 1)[-1] in ('gamma1', 'gamma2')]
    assert len(gammas) == 6 and all(where[k] == [] for k in gammas), {k: where[k] for k in gammas}
    assert all(m.get_parameter(k).requires_grad for k in gammas)
    assert where['model.5.dwconv.bias'] == [2] and where['model.5.pws.2.weight'] == [1]


def test_refusals():
    from dmayolo.models import common as P
    with pytest.raises(NotImplementedError, match='gflayer'):
        P.GnConv(64, 64, gflayer=object())
    with pytest.raises(NotImplementedError, match='drop_path'):
        P.HorBlock(64, drop_path=0.1)
    with pytest.raises(NotImplementedError):
        P.LayerNorm(64, data_format='channels_middle')
    assert P.HorBlock(64, layer_scale_init_value=0).gamma1 is None
    assert P.HorBlock(64, layer_scale_init_value=0).gamma2 is None


@pytest.mark.parametrize('c1,dtype', [(64, torch.bfloat16), (32, torch.float32), (72, torch.float32)],
                         ids=['bf16-64', 'fp32-32', 'fp32-72'])
def test_narrow_gnconv_is_refused_before_any_launch(c1, dtype):
    """every gate width must be a whole 16-byte vector: c1 >= 128 in bf16, >= 64 in fp32, c1 % 16 == 0.  The check runs
    before any kernel: a CPU tensor reaches it"""
    from dmayolo.models import common as P
    x = torch.zeros(1, c1, 8, 8, dtype=dtype).contiguous(memory_format=CL)
    for mod in (P.GnConv(c1, c1), P.HorBlock(c1), P.C3HB(2 * c1, 2 * c1).m):
        with pytest.raises(NotImplementedError, match=rf'GnConv: c1={c1} .*{dtype}'):
            mod(x)
