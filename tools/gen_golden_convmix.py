"""Capture the reference's ConvMixer family (models/cspcm.py:25-54, ConvMix and CSPCM) on its own PyTorch-CPU path in
fp32 with 8 intra-op threads (in-container only, like tools/gen_golden_hor.py).  Only data is written, none of the
reference's code.

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_convmix.py [dw9 modules model]
  dw9.npz          nn.Conv2d(C, C, 9, groups=C, padding='same') alone, the first layer of ConvMix.Resnet, at (N, C, H, W)
                   = (2, 8, 5, 7) (the whole map inside the halo), (1, 24, 9, 13) (three channel units, W no multiple of
                   the strip) and (2, 16, 12, 18): keys '<i>.x / w / b / dz' (inputs) and '.y / dx / dw / db' (the output
                   and the gradients of sum(y * dz))
  convmix.npz      ConvMix(64, 64) on (2, 64, 10, 12): tools/gen_golden.py's module keys (train step and eval forward); BN
  cspcm.npz        weight ~ U(0.5, 1.5), bias / running_mean ~ N(0, 0.1^2), running_var ~ U(0.5, 1.5), conv biases as
                   initialised.  CSPCM(64, 128, 1) on the same input
  cspcm_model.npz  a cut-down CSPCM.yaml (MODEL_YAML below: every depthwise layer 32 or 128 wide, a 64 px input so the
                   P5 map is 2 x 2 and the P4 map 4 x 4, both under the 9 x 9 filter), width 1.0, nc 10, batch 2,
                   hor_model.npz's keys.  Its meta also holds, for each of the reference's five model files that name
                   the family, the module lists retyped as data and what the reference's own parse_model makes of
                   them: layer count, per-layer module names, its per-layer channel list, repeat counts, parameter counts
                   and the strides of its 256 px probe (None where the reference itself cannot run it)
"""
import json
import os
import sys

from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the import shim, imports the reference)

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
from adapt_ref import fill_state_dict  # noqa: E402
import models.cspcm as CM  # noqa: E402  (reference)

Y, OUT, npy = G.Y, G.OUT, G.npy
SHAPES = [(2, 8, 5, 7), (1, 24, 9, 13), (2, 16, 12, 18)]  # (N, C, H, W)
YAMLS = ['CSPCM.yaml', 'ConvMix.yaml', 'CMCA.yaml', 'yolo_cspcm.yaml', 'yolo_convmix.yaml']


def gen_dw9():
    d, gen = {}, torch.Generator().manual_seed(909)
    for i, (N, ch, H, W) in enumerate(SHAPES):
        m = nn.Conv2d(ch, ch, kernel_size=9, groups=ch, padding='same')
        with torch.no_grad():
            m.weight.copy_(torch.randn(ch, 1, 9, 9, generator=gen) / 9)
            m.bias.copy_(torch.randn(ch, generator=gen))
        x = torch.randn(N, ch, H, W, generator=gen).requires_grad_(True)
        dz = torch.randn(N, ch, H, W, generator=gen)
        y = m(x)
        (y * dz).sum().backward()
        for k, v in (('x', x), ('w', m.weight), ('b', m.bias), ('dz', dz), ('y', y), ('dx', x.grad),
                     ('dw', m.weight.grad), ('db', m.bias.grad)):
            d[f'{i}.{k}'] = npy(v)
    meta = dict(module='nn.Conv2d', args=['C', 'C', 9], kwargs=dict(groups='C', padding='same'), shapes=SHAPES)
    np.savez_compressed(os.path.join(OUT, 'dw9.npz'), meta=json.dumps(meta), **d)
    print('wrote dw9', sum(v.nbytes for v in d.values()) / 1e6, 'MB')


def gen_modules():
    torch.manual_seed(90)
    for i, (name, cls, args) in enumerate((('convmix', 'ConvMix', [64, 64]), ('cspcm', 'CSPCM', [64, 128, 1]))):
        G.module_case(name, getattr(CM, cls)(*args), [G.rnd(2, 64, 10, 12, seed=91 + i)], dict(module=cls, args=args),
                      seed=91 + i)
        path = os.path.join(OUT, f'{name}.npz')
        print(name, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 2 ** 20


ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
MODEL_YAML = dict(
    nc=10, depth_multiple=1.0, width_multiple=1.0, anchors=ANCHORS,
    backbone=[[-1, 1, 'Conv', [32, 6, 2, 2]],         # 0 stem, P1/2
              [-1, 1, 'Conv', [32, 3, 1]],            # 1
              [-1, 1, 'space_to_depth', [1]],         # 2 P2/4, 128 channels
              [-1, 1, 'Conv', [64, 3, 2]],            # 3 P3/8
              [-1, 1, 'C3', [64]],                    # 4
              [-1, 1, 'Conv', [64, 3, 2]],            # 5 P4/16
              [-1, 1, 'space_to_depth', [1]],         # 6 P5/32, 256 channels
              [-1, 2, 'CSPCM', [256]],                # 7 two CSPCM(256, 256) in sequence (n is not inserted), c_ = 128
              [-1, 1, 'SPPF', [128, 5]]],             # 8
    head=[[-1, 1, 'Conv', [64, 1, 1]],                # 9
          [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
          [[-1, 5], 1, 'Concat', [1]],                # 11 cat backbone P4
          [-1, 1, 'CSPCM', [64]],                     # 12 c_ = 32
          [[4, 12, 8], 1, 'Detect', ['nc', 'anchors']]])


def _meta(model, yml, nc, img):
    return dict(yaml=yml, nc=nc, img=img, stride=[float(s) for s in model.stride],
                sd_shapes={k: list(v.shape) for k, v in model.state_dict().items()})


def _yaml_numbers():
    """names and numbers of the reference's five model files that name ConvMix / CSPCM, built by its own parse_model"""
    import yaml
    out = {}
    for f in YAMLS:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(CM.__file__))), 'models', f)
        with open(path, errors='ignore') as fh:
            d = yaml.safe_load(fh)
        seen = {}

        def prof(frame, event, arg):  # parse_model's own channel bookkeeping: its local `ch` as it returns
            if event == 'return' and frame.f_code.co_name == 'parse_model':
                seen['ch'] = [int(c) for c in frame.f_locals['ch']]
        sys.setprofile(prof)
        try:
            layers, _ = Y.parse_model(deepcopy(d), ch=[3])  # the layer list alone: no stride probe
        finally:
            sys.setprofile(None)
        assert len(seen['ch']) == len(layers)
        try:  # whether the reference's own Model runs its 256 px stride probe on this file
            probe = [float(v) for v in Y.Model(deepcopy(d), ch=3).stride]
        except RuntimeError as e:
            probe = None
            print(f, 'does not pass the stride probe of the reference:', str(e)[:100])
        out[f] = dict(layers=len(layers), types=[m.type.rsplit('.', 1)[-1] for m in layers], stride=probe,
                      channels=seen['ch'],
                      np=[int(m.np) for m in layers], params=int(sum(p.numel() for p in layers.parameters())),
                      repeats=[len(m) if isinstance(m, nn.Sequential) and m.type.endswith(('CSPCM', 'ConvMix')) else 0
                               for m in layers],
                      sd_keys=len(layers.state_dict()),
                      **{k: d[k] for k in ('nc', 'depth_multiple', 'width_multiple', 'anchors')},
                      backbone=d['backbone'], head=d['head'])
    return out


def gen_model():
    name, yml, nc, img, bs, seed = 'cspcm_model', deepcopy(MODEL_YAML), 10, 64, 2, 191
    torch.manual_seed(seed)
    model = fill_state_dict(Y.Model(deepcopy(yml), nc=nc))
    print(name, sum(p.numel() for p in model.parameters()) / 1e6, 'M parameters')
    assert [float(s) for s in model.stride] == [8.0, 16.0, 32.0]
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randint(0, 256, (bs, 3, img, img), generator=torch.Generator().manual_seed(seed + 2)).float() / 255
    model.train()
    outs = model(x)
    gups = [torch.randn(o.shape, generator=gen) * 0.1 for o in outs]
    sum((o * g).sum() for o, g in zip(outs, gups)).backward()
    meta = _meta(model, yml, nc, img)
    meta['yamls'] = _yaml_numbers()
    d = {'meta': json.dumps(meta), 'in.0': npy(x)}
    for k, v in sd0.items():  # what fill_state_dict does not give: Detect's anchors in grid units
        if k.endswith('anchors'):
            d[f'sd.{k}'] = npy(v)
    for i, (o, g) in enumerate(zip(outs, gups)):
        d[f'out.{i}'] = npy(o)
        d[f'gup.{i}'] = npy(g)
    params = dict(model.named_parameters())
    blk = next(k for k, m in model.named_modules() if isinstance(m, CM.ConvMix))
    own = [k for k in params if k.startswith(blk + '.') and params[k].numel() < 4096]
    small = [k for k in params if '.m.' in k and params[k].dim() == 1 and 'Resnet' in k or 'Conv_1x1.0.bias' in k]
    assert own and all(p.grad is not None for p in params.values())
    for k in dict.fromkeys(list(params)[:6] + list(params)[-6:] + own + small):
        d[f'gp.{k}'] = npy(params[k].grad)
    d['gnorm'] = np.array([float(p.grad.norm()) for p in params.values()], dtype=np.float64)
    d['pnames'] = np.array(list(params.keys()))
    model.load_state_dict(sd0)
    model.eval()
    with torch.no_grad():
        z, _ = model(x)
    d['eval_out'] = npy(z)
    path = os.path.join(OUT, f'{name}.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 2 ** 20


if __name__ == '__main__':
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ['dw9', 'modules', 'model']:
        globals()[f'gen_{w}']()
