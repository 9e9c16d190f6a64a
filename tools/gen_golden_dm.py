"""Capture the reference's SPD-mix downsamplers (models/common.py:1460-1475 SM / MP, 1508-1547 DMMConv2 / DMMConv /
DMConv) on its own PyTorch-CPU path in fp32 (in-container only, like tools/gen_golden_adapt.py).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_dm.py
Writes, under tests/golden/ (data only, none of the reference's code):
  dmconv / dmmconv / dmmconv2 .npz   tools/gen_golden.py's module keys, (16, 24) modules on a (2, 16, 12, 20) input
  dm_model_cadmm.npz    CADMM.yaml's layer list, every width divided by 8
  dm_model_cadmm2.npz   CADMM2.yaml's layer list, every width divided by 8
  dm_model_dm.npz       DM.yaml's layer list divided by 8: meta only (names, shapes, strides; build test)
8 is the largest divisor that keeps every layer on a bf16 vector multiple (the stem and the narrowest C3 halves have 8
channels).  The model fixtures use adapt_model_*.npz's keys: the weights come from tests/adapt_ref.py::fill_state_dict,
which the tests call too (sd.* holds only Detect's anchors).
"""
import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the import shim, imports the reference)

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
from adapt_ref import fill_state_dict  # noqa: E402

Y, C, OUT, npy = G.Y, G.C, G.OUT, G.npy
_WIDTH = ('Conv', 'C3', 'C3CA', 'SPPF', 'DMConv', 'DMMConv', 'DMMConv2')
DIV = 8


def reduced_yaml(name, div=DIV):
    """the reference YAML's layer list with every channel argument divided by div"""
    import yaml
    d = yaml.safe_load(open(os.path.join(G.ref_stubs.REF, 'models', name)))
    for l in d['backbone'] + d['head']:
        if l[2] in _WIDTH:
            l[3][0] //= div
    d['depth_multiple'], d['width_multiple'], d['nc'] = 0.33, 1.0, 10
    return d


def _meta(model, yml, nc, img):
    return dict(yaml=yml, nc=nc, img=img, stride=[float(s) for s in model.stride],
                sd_shapes={k: list(v.shape) for k, v in model.state_dict().items()})


def gen_model():
    for name, src, seed in (('dm_model_cadmm', 'CADMM.yaml', 71), ('dm_model_cadmm2', 'CADMM2.yaml', 81)):
        yml, nc, img, bs = reduced_yaml(src), 10, 64, 2
        torch.manual_seed(seed)
        model = fill_state_dict(Y.Model(deepcopy(yml), nc=nc))
        print(name, sum(p.numel() for p in model.parameters()) / 1e6, 'M parameters')
        assert [float(s) for s in model.stride] == [4.0, 8.0, 16.0, 32.0]
        sd0 = {k: v.clone() for k, v in model.state_dict().items()}
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randint(0, 256, (bs, 3, img, img), generator=torch.Generator().manual_seed(seed + 2)).float() / 255
        model.train()
        outs = model(x)
        gups = [torch.randn(o.shape, generator=gen) * 0.1 for o in outs]
        sum((o * g).sum() for o, g in zip(outs, gups)).backward()
        d = {'meta': json.dumps(_meta(model, yml, nc, img)), 'in.0': npy(x)}
        for k, v in sd0.items():  # what fill_state_dict leaves alone: Detect's anchors in grid units
            if k.endswith('anchors'):
                d[f'sd.{k}'] = npy(v)
        for i, (o, g) in enumerate(zip(outs, gups)):
            d[f'out.{i}'] = npy(o)
            d[f'gup.{i}'] = npy(g)
        params = dict(model.named_parameters())
        dm = [k for k, m in model.named_modules() if isinstance(m, (C.DMConv, C.DMMConv, C.DMMConv2))]
        own = [k for k in params if any(k.startswith(f + '.') for f in dm) and params[k].grad is not None]
        assert own
        for k in dict.fromkeys(list(params)[:6] + list(params)[-6:] + own):
            d[f'gp.{k}'] = npy(params[k].grad)
        d['gnorm'] = np.array([float(p.grad.norm()) if p.grad is not None else 0.0 for p in params.values()],
                              dtype=np.float64)
        d['pnames'] = np.array(list(params.keys()))
        model.load_state_dict(sd0)
        model.eval()
        with torch.no_grad():
            z, _ = model(x)
        d['eval_out'] = npy(z)
        path = os.path.join(OUT, f'{name}.npz')
        np.savez_compressed(path, **d)
        print('wrote', path, os.path.getsize(path), 'bytes')
    yml = reduced_yaml('DM.yaml')
    model = Y.Model(deepcopy(yml), nc=10)
    np.savez_compressed(os.path.join(OUT, 'dm_model_dm.npz'), meta=json.dumps(_meta(model, yml, 10, 64)))


def gen_modules():
    torch.manual_seed(70)
    for i, (name, cls) in enumerate((('dmconv', 'DMConv'), ('dmmconv', 'DMMConv'), ('dmmconv2', 'DMMConv2'))):
        G.module_case(name, getattr(C, cls)(16, 24), [G.rnd(2, 16, 12, 20, seed=91 + i)],
                      dict(module=cls, args=[16, 24]), seed=91 + i)


if __name__ == '__main__':
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ['modules', 'model']:
        globals()[f'gen_{w}']()
