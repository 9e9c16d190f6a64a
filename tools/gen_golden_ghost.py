"""Capture the reference's Ghost modules (models/common.py:79-82, 666-699, 205-210) on its own PyTorch-CPU path in
fp32 (in-container only, like tools/gen_golden.py): GhostBottleneck alone at stride 1 and 2, and a small
yolov5s-ghost (models/hub/yolov5s-ghost.yaml's layer list with the v6.0 stem in place of Focus, the same map).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_ghost.py
Writes tests/golden/ghostbottleneck_s1.npz, ghostbottleneck_s2.npz (tools/gen_golden.py's module keys) and
tests/golden/ghost_v5s.npz (model_v5s.npz's keys, plus gp.* of every depthwise weight and eval_out): data only,
none of the reference's code.
"""
import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (installs the import shim, imports the reference)

Y, C, OUT, npy = G.Y, G.C, G.OUT, G.npy

STEM = [-1, 1, 'Conv', [64, 6, 2, 2]]  # v6.0 stem; the hub yaml's Focus [64, 3] computes the same map


def ghost_yaml():
    """hub/yolov5s-ghost.yaml's layers; every stage width 128 except the last backbone stage, SPP and the P5 head
    (256), so that with width_multiple 0.5 the narrowest depthwise layer has 8 channels"""
    import yaml
    d = yaml.safe_load(open(os.path.join(G.ref_stubs.REF, 'models', 'hub', 'yolov5s-ghost.yaml')))
    layers = d['backbone'] + d['head']
    assert layers[0][2] == 'Focus'
    d['backbone'][0] = list(STEM)
    wide = {7, 8, 9, 23}
    for i, l in enumerate(d['backbone'] + d['head']):
        if i and l[2] in ('GhostConv', 'C3Ghost', 'SPP'):
            l[3][0] = 256 if i in wide else 128
    d['depth_multiple'], d['width_multiple'] = 0.33, 0.5
    return d


def gen_model():
    yml, nc, img, bs = ghost_yaml(), 10, 64, 2
    torch.manual_seed(21)
    model = Y.Model(deepcopy(yml), nc=nc)
    dws = [k + '.weight' for k, m in model.named_modules()
           if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    assert dws and all(m.groups == m.in_channels == m.out_channels for m in model.modules()
                       if isinstance(m, torch.nn.Conv2d) and m.groups > 1)
    print('depthwise layers', len(dws), 'narrowest', min(model.state_dict()[k].shape[0] for k in dws), 'channels')
    assert min(model.state_dict()[k].shape[0] for k in dws) == 8
    assert [float(s) for s in model.stride] == [8.0, 16.0, 32.0]
    gen = torch.Generator().manual_seed(22)
    G.randomize_bn(model, gen)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if v.dtype.is_floating_point:
                v.copy_(v.half().float())
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    # an 8-bit image scaled to [0, 1]: 256 distinct values, which keeps the compressed fixture under 1 MiB
    x = torch.randint(0, 256, (bs, 3, img, img), generator=torch.Generator().manual_seed(23)).float() / 255
    model.train()
    outs = model(x)
    gups = [torch.randn(o.shape, generator=gen) * 0.1 for o in outs]
    sum((o * g).sum() for o, g in zip(outs, gups)).backward()
    d = {'meta': json.dumps(dict(yaml=yml, nc=nc, img=img)), 'in.0': npy(x)}
    for k, v in sd0.items():
        d[f'sd.{k}'] = v.half().numpy() if v.dtype.is_floating_point else npy(v)
    for i, (o, g) in enumerate(zip(outs, gups)):
        d[f'out.{i}'] = npy(o)
        d[f'gup.{i}'] = npy(g)
    params = dict(model.named_parameters())
    for k in dict.fromkeys(list(params)[:6] + list(params)[-6:] + dws):
        d[f'gp.{k}'] = npy(params[k].grad)
    d['gnorm'] = np.array([float(p.grad.norm()) if p.grad is not None else 0.0 for p in params.values()],
                          dtype=np.float64)
    d['pnames'] = np.array(list(params.keys()))
    model.load_state_dict(sd0)
    model.eval()
    with torch.no_grad():
        z, _ = model(x)
    d['eval_out'] = npy(z)
    path = os.path.join(OUT, 'ghost_v5s.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path), 'bytes')


def gen_modules():
    for s in (1, 2):
        G.module_case(f'ghostbottleneck_s{s}', C.GhostBottleneck(32, 32, 3, s), [G.rnd(2, 32, 13, 17, seed=40 + s)],
                      dict(module='GhostBottleneck', args=[32, 32, 3, s]), seed=40 + s)


if __name__ == '__main__':
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ['modules', 'model']:
        globals()[f'gen_{w}']()
