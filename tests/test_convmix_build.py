"""CPU: parse_model builds YAMLs naming ConvMix / CSPCM with the reference's parameter names, order, shapes and counts;
the no-insertion-of-n rule, the optimizer grouping and Model.fuse().  No kernel runs here."""
import copy

import pytest
import torch
import torch.nn as nn

from golden_util import Fixture

YAMLS = ['CSPCM.yaml', 'ConvMix.yaml', 'CMCA.yaml', 'yolo_cspcm.yaml', 'yolo_convmix.yaml']


def _cfg(rec):
    return {k: copy.deepcopy(rec[k]) for k in ('nc', 'depth_multiple', 'width_multiple', 'anchors', 'backbone', 'head')}


def _build(yaml):
    from dmayolo.models.yolo import Model
    return Model(copy.deepcopy(yaml), nc=10)


def test_product_builds_fixture_yaml():
    fx = Fixture('cspcm_model')
    m, meta = _build(fx.meta['yaml']), fx.meta
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    want = meta['sd_shapes']
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    assert sd == want, [k for k in sd if sd[k] != want[k]]
    assert list(sd) == list(want)  # the reference's order
    assert [float(s) for s in m.stride] == meta['stride'] == [8.0, 16.0, 32.0]
    assert [str(s) for s in fx.z['pnames']] == [k for k, _ in m.named_parameters()]
    from dmayolo.models import common as P
    assert isinstance(m.model[7], nn.Sequential) and [type(b) for b in m.model[7]] == [P.CSPCM, P.CSPCM]
    assert type(m.model[12]) is P.CSPCM and m.model[12].m[0].Resnet[0].groups == 32
    assert m.model[7][0].m[0].Resnet[0].kernel_size == (9, 9) and m.model[7][0].m[0].Resnet[0].bias is not None


def test_module_keys_match_the_reference():
    from dmayolo.models import common as P
    for name in ('convmix', 'cspcm'):
        fx = Fixture(name)
        want = fx.group('sd')
        sd = getattr(P, fx.meta['module'])(*fx.meta['args']).state_dict()
        assert list(sd) == list(want) and all(sd[k].shape == want[k].shape for k in sd), name
    assert 'ConvMix' in P.__all__ and 'CSPCM' in P.__all__
    keys = list(P.ConvMix(64, 64).state_dict())
    assert keys[:2] == ['Resnet.0.weight', 'Resnet.0.bias'] and 'Resnet.2.running_var' in keys
    assert 'Conv_1x1.0.bias' in keys and 'Conv_1x1.2.weight' in keys
    c = P.CSPCM(64, 128, 2)
    assert isinstance(c, P.C3) and len(c.m) == 2 and {k.split('.')[0] for k in c.state_dict()} == {'cv1', 'cv2', 'cv3', 'm'}
    for st in (c.m[0].Resnet, c.m[0].Conv_1x1):
        assert isinstance(st, nn.Sequential) and [type(l) for l in st] == [nn.Conv2d, nn.GELU, nn.BatchNorm2d]


@pytest.mark.parametrize('name', YAMLS)
def test_parse_model_matches_the_reference_on_the_five_yamls(name):
    """layer count, per-layer module names, the per-layer channel list, per-layer and total parameter counts and the
    repeat structure recorded from the reference's own parse_model (names and numbers only).  The channel list is
    parse_model's own bookkeeping (its `ch` as it returns), which also covers the layers without parameters and the
    reference's rule that a YAML-level ConvMix records the width-scaled args[0] as its output"""
    import sys
    from dmayolo.models.yolo import parse_model
    rec = Fixture('cspcm_model').meta['yamls'][name]
    d = _cfg(rec)
    seen = {}

    def prof(frame, event, arg):
        if event == 'return' and frame.f_code.co_name == 'parse_model':
            seen['ch'] = [int(c) for c in frame.f_locals['ch']]
    sys.setprofile(prof)
    try:
        layers, _ = parse_model(d, [3])
    finally:
        sys.setprofile(None)
    assert len(layers) == rec['layers']
    assert seen['ch'] == rec['channels']
    from dmayolo.models import common as P
    for l, c2 in zip(layers, rec['channels']):  # and what the built layers with parameters really emit
        last = l[-1] if isinstance(l, torch.nn.Sequential) and not isinstance(l, P.ConvMix) and len(l) and \
            isinstance(l[-1], (P.CSPCM, P.ConvMix)) else l
        if isinstance(last, P.C3):
            assert last.cv3.conv.out_channels == c2
        elif isinstance(last, P.ConvMix):
            assert last.Conv_1x1[0].out_channels == last.Resnet[0].in_channels  # emits c1 whatever was recorded
        elif isinstance(last, P.Conv):
            assert last.conv.out_channels == c2
    assert [l.type.rsplit('.', 1)[-1] for l in layers] == rec['types']
    assert [int(l.np) for l in layers] == rec['np']
    assert sum(p.numel() for p in layers.parameters()) == rec['params']
    assert len(layers.state_dict()) == rec['sd_keys']
    rep = [len(l) if isinstance(l, nn.Sequential) and l.type.endswith(('CSPCM', 'ConvMix')) else 0 for l in layers]
    assert rep == rec['repeats'] and any(t in ('CSPCM', 'ConvMix') for t in rec['types'])


@pytest.mark.parametrize('name', YAMLS)
def test_model_builds_the_yamls_the_reference_can_run(name):
    """Model() on the module lists: the stride walk gives the strides of the reference's 256 px probe.  CMCA.yaml does
    not pass that probe in the reference itself (its Concat inputs differ in size), so there is nothing to compare"""
    from dmayolo.models.yolo import Model
    rec = Fixture('cspcm_model').meta['yamls'][name]
    if rec['stride'] is None:
        assert name == 'CMCA.yaml'
        return
    m = Model(_cfg(rec))
    assert [float(s) for s in m.stride] == rec['stride'] == [4.0, 8.0, 16.0, 32.0]
    assert sum(p.numel() for p in m.parameters()) == rec['params']
    assert len(m.state_dict()) == rec['sd_keys']


def test_n_is_not_inserted():
    """models/yolo.py:409-413: [-1, 3, CSPCM, [4096]] is three CSPCM(c1, c2) with one ConvMix each, not CSPCM(n=3)"""
    from dmayolo.models import common as P
    from dmayolo.models.yolo import parse_model
    d = {'nc': 10, 'anchors': 3, 'depth_multiple': 1.0, 'width_multiple': 0.25,
         'backbone': [[-1, 1, 'Conv', [128, 3, 1]], [-1, 3, 'CSPCM', [128]], [-1, 2, 'ConvMix', [128]]], 'head': []}
    layers, _ = parse_model(d, [3])
    assert isinstance(layers[1], nn.Sequential) and len(layers[1]) == 3
    assert all(type(b) is P.CSPCM and len(b.m) == 1 and b.cv1.conv.in_channels == 32 for b in layers[1])
    assert isinstance(layers[2], nn.Sequential) and len(layers[2]) == 2 and type(layers[2][0]) is P.ConvMix
    assert layers[2][0].Resnet[0].in_channels == 32


def test_param_groups_and_fuse():
    """train.py:197-214: conv biases and BN biases in the bias group, BN weights in the no-decay group, conv weights
    decayed; Model.fuse() leaves ConvMix's convs unfused, as the reference does"""
    from dmayolo.optim import param_groups
    m = _build(Fixture('cspcm_model').meta['yaml'])
    g0, g1, g2 = param_groups(m)
    ids = [{id(p) for p in g} for g in (g0, g1, g2)]
    where = {k: [i for i, s in enumerate(ids) if id(p) in s] for k, p in m.named_parameters()}
    for blk in ('model.7.0.m.0.', 'model.7.1.m.0.', 'model.12.m.0.'):
        for st in ('Resnet', 'Conv_1x1'):
            assert where[f'{blk}{st}.0.weight'] == [1] and where[f'{blk}{st}.0.bias'] == [2]
            assert where[f'{blk}{st}.2.weight'] == [0] and where[f'{blk}{st}.2.bias'] == [2]
    assert all(len(v) == 1 for v in where.values())
    before = list(m.state_dict())
    m.fuse()
    mix = m.model[12].m[0]
    assert isinstance(mix.Resnet[2], nn.BatchNorm2d) and isinstance(mix.Conv_1x1[2], nn.BatchNorm2d)
    assert [k for k in before if '.m.0.Resnet.' in k or '.m.0.Conv_1x1.' in k] == \
        [k for k in m.state_dict() if '.m.0.Resnet.' in k or '.m.0.Conv_1x1.' in k]
