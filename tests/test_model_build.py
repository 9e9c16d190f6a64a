"""CPU: the drop-in Model/parse_model builds the reference YAMLs with identical state_dict keys,
shapes and parameter counts (the plugin boundary, models/yolo.py:353-478)."""
import os

import pytest
import torch
import yaml

from golden_util import Fixture

YAMLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dma-yolo_amd', 'dmayolo', 'configs')


@pytest.mark.parametrize('name', ['model_v5s', 'model_dma', 'model_c5'])
def test_state_dict_matches_reference(name):
    from dmayolo.models.yolo import Model
    fx = Fixture(name)
    m = Model(fx.meta['yaml'], nc=fx.meta['nc'])
    sd = m.state_dict()
    ref = fx.group('sd')
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k


@pytest.mark.parametrize('cfg,nc,params', [('yolov5s.yaml', 10, 7046599), ('yolov5n.yaml', 80, 1872157),
                                           ('yolov5l-ca-sppfcspc-bifpn-scconv.yaml', 10, 81276228)])
def test_param_counts(cfg, nc, params):
    from dmayolo.models.yolo import Model
    m = Model(os.path.join(YAMLS, cfg), nc=nc)
    assert sum(p.numel() for p in m.parameters()) == params
    det = m.model[-1]
    assert det.stride.tolist() == [8.0, 16.0, 32.0]
    # BN defaults applied (utils/torch_utils.py:161-170)
    bns = [b for b in m.modules() if type(b) is torch.nn.BatchNorm2d]
    assert bns and all(b.eps == 1e-3 and b.momentum == 0.03 for b in bns)


def test_optimizer_groups_match_reference():
    from dmayolo.models.yolo import Model
    from dmayolo.optim import param_groups
    fx = Fixture('optim')
    groups = fx.meta['groups']
    m = Model(fx.meta['yaml'], nc=3)
    names = {id(p): k for k, p in m.named_parameters()}
    g0, g1, g2 = param_groups(m)
    assert [names[id(p)] for p in g0] == groups['g0']
    assert [names[id(p)] for p in g1] == groups['g1']
    assert [names[id(p)] for p in g2] == groups['g2']


def test_caspd_tdetect_layout_matches_reference():
    """CASPD_ODRTA (space_to_depth + C3CA + TDetect P2-P5): parameter count, state_dict shapes, strides."""
    from dmayolo.models.yolo import Model
    fx = Fixture('model_caspd_layout')
    m = Model(os.path.join(YAMLS, 'CASPD_ODRTA.yaml'), nc=fx.meta['nc'])
    sd = m.state_dict()
    ref = fx.meta['shapes']
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    for k, v in ref.items():
        assert list(sd[k].shape) == v, k
    assert sum(p.numel() for p in m.parameters()) == fx.meta['nparams']
    assert [float(s) for s in m.stride] == fx.meta['stride']


def test_config5_layout_matches_reference():
    """yolov5l-xs-tr-cbam-spp-bifpn.yaml (C3TR + CBAM + SPP, 4-level Detect with `anchors: 4`): parameter
    count, state_dict shapes, strides and the placeholder anchors (models/yolo.py:432-436)."""
    from dmayolo.models.yolo import Model
    fx = Fixture('model_c5_layout')
    m = Model(os.path.join(YAMLS, 'yolov5l-xs-tr-cbam-spp-bifpn.yaml'), nc=fx.meta['nc'])
    sd = m.state_dict()
    ref = fx.meta['shapes']
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    for k, v in ref.items():
        assert list(sd[k].shape) == v, k
    assert sum(p.numel() for p in m.parameters()) == fx.meta['nparams'] == 60401284
    assert [float(s) for s in m.stride] == fx.meta['stride']
    assert m.model[-1].anchors.tolist() == fx.meta['anchors']


def test_config5_in_proj_never_optimized():
    """train.py:197-214 grouping collects .weight/.bias attributes only: the 12 MHA in_proj params
    (4,727,808 values) get gradients but never enter the optimizer."""
    from dmayolo.models.yolo import Model
    from dmayolo.optim import param_groups
    m = Model(os.path.join(YAMLS, 'yolov5l-xs-tr-cbam-spp-bifpn.yaml'), nc=3)
    grouped = {id(p) for g in param_groups(m) for p in g}
    missing = [(k, p.numel()) for k, p in m.named_parameters() if id(p) not in grouped]
    assert len(missing) == 12 and all('in_proj' in k for k, _ in missing), missing
    assert sum(n for _, n in missing) == 4727808


@pytest.mark.parametrize('cfg,plan', [('yolov5l-ca-sppfcspc-bifpn-scconv.yaml', {4: 2, 6: 3, 10: 2, 14: 2, 18: 2, 21: 2}),
                                      ('yolov5s.yaml', {4: 2, 6: 2, 17: 2, 20: 2})])
def test_gradient_fanout_plan(cfg, plan):
    """Model-level GradSinks: the layer outputs read by >= 2 layers of which >= 1 takes a sink (BiFPN skips, the
    P3-P5 outputs read by a Conv and Detect); outputs read only by Upsample / plain Concat stay with autograd, and
    Detect joins only under DMY_SINK_DETECT=1"""
    from dmayolo.models.yolo import Model
    import dmayolo.functional as Fn
    m = Model(os.path.join(YAMLS, cfg), nc=10)
    assert m._fanout() == plan
    # consumers register their contributions in forward: SCConv 3, a Conv / Detect level / AdConcat slot 1 each
    sinks = {i: Fn.GradSink(0) for i in plan}
    for layer in m.model:
        m._sink_kw(layer, sinks)
        name = type(layer).__name__
        if name == 'SCConv':  # SCConv.forward joins its own three
            src = layer.f if layer.f != -1 else layer.i - 1
            if src in sinks:
                sinks[src].expect(3)
        elif name in ('AdConcat2', 'AdConcat3') or (name == 'Detect' and name in m._SINK_TYPES):
            for j in layer.f:
                j = layer.i - 1 if j == -1 else j
                if j in sinks:
                    sinks[j].expect(1)
    aware = {i: sum(1 for layer in m.model for j in ([layer.f] if isinstance(layer.f, int) else layer.f)
                    if (layer.i - 1 if j == -1 else j) == i and type(layer).__name__ in m._SINK_TYPES)
             for i in plan}
    for i, sk in sinks.items():
        n_scconv = sum(2 for layer in m.model if type(layer).__name__ == 'SCConv' and
                       (layer.f if layer.f != -1 else layer.i - 1) == i)
        assert sk.n == aware[i] + n_scconv, (i, sk.n)


def test_out_view_rule():
    """functional.out_view, the output-into-slice rule shared by ConvBNActFn, MaxPoolFn, ResizeFn and maxpool_chain3:
    a view is written in place only with the result's shape, dtype and device and NHWC-addressable as it stands"""
    from dmayolo.functional import out_view
    buf = torch.zeros(2, 32, 4, 4).contiguous(memory_format=torch.channels_last)
    like = torch.zeros(1)
    sl = buf[:, 8:24]
    v, ps = out_view(sl, (2, 16, 4, 4), like)
    assert v is sl and ps == 32
    assert out_view(None, (2, 16, 4, 4), like) == (None, None)
    assert out_view(sl, (2, 16, 4, 2), like) == (None, None)  # wrong shape
    assert out_view(sl, (2, 16, 4, 4), like.bfloat16()) == (None, None)  # another dtype
    assert out_view(torch.zeros(2, 32, 4, 4)[:, 8:24], (2, 16, 4, 4), like) == (None, None)  # NCHW-contiguous buffer
    # a [::2] batch slice: two images twice the image size apart are not addressable in place.  (Out of the batch-2
    # buffer above the same slice keeps ONE image, which any batch stride addresses: that one is rightly accepted.)
    buf4 = torch.zeros(4, 32, 4, 4).contiguous(memory_format=torch.channels_last)
    assert out_view(buf4[::2, 8:24], (2, 16, 4, 4), like) == (None, None)
    assert out_view(buf[::2, 8:24], (1, 16, 4, 4), like)[1] == 32
