"""Capture the reference's adaptive-fusion modules (models/common.py:953-992 AdaptConcat, 1028-1061 Adapt_Add2 /
Adapt_Add3, 1063-1081 add_conv) on its own PyTorch-CPU path in fp32 (in-container only, like tools/gen_golden.py).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_adapt.py
Writes, under tests/golden/ (data only, none of the reference's code):
  adaptconcat_l2 / adaptconcat_l3 / adapt_add2 / adapt_add3 .npz   tools/gen_golden.py's module keys
  adapt_model_ca.npz    adaptca.yaml's layer list, every width (the AdaptConcat dims included) divided by 4
  adapt_model_spd6.npz  C3CASPD6.yaml's layer list, every width (the Adapt_Add3 dims included) divided by 8
  adapt_model_str.npz   adaptconcat.yaml's layer list divided by 2: meta only (names, shapes, strides; build test)
The model fixtures use ghost_v5s.npz's keys: the weights come from tests/adapt_ref.py::fill_state_dict, which the
tests call too (sd.* holds only Detect's anchors).  meta carries the edited YAML dict, the state_dict's shapes and
the strides.
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
_WIDTH = ('Conv', 'C3', 'C3CA', 'C3STR', 'SPPF')


def reduced_yaml(name, div):
    """the reference YAML's layer list with every channel argument divided by div"""
    import yaml
    d = yaml.safe_load(open(os.path.join(G.ref_stubs.REF, 'models', name)))
    for l in d['backbone'] + d['head']:
        if l[2] in _WIDTH:
            l[3][0] //= div
        elif l[2] == 'AdaptConcat':
            l[3][1:] = [c // div for c in l[3][1:]]
        elif l[2] == 'Adapt_Add3':
            l[3] = [c // div for c in l[3]]
    d['depth_multiple'], d['width_multiple'], d['nc'] = 0.33, 1.0, 10
    return d


def _meta(model, yml, nc, img):
    return dict(yaml=yml, nc=nc, img=img, stride=[float(s) for s in model.stride],
                sd_shapes={k: list(v.shape) for k, v in model.state_dict().items()})


def gen_model():
    for name, src, div, seed in (('adapt_model_ca', 'adaptca.yaml', 4, 31), ('adapt_model_spd6', 'C3CASPD6.yaml', 8, 41)):
        yml, nc, img, bs = reduced_yaml(src, div), 10, 64, 2
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
        fusion = [k for k, m in model.named_modules() if isinstance(m, (C.AdaptConcat, C.Adapt_Add2, C.Adapt_Add3))]
        own = [k for k in params if any(k.startswith(f + '.') for f in fusion) and params[k].grad is not None]
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
    yml = reduced_yaml('adaptconcat.yaml', 2)
    model = Y.Model(deepcopy(yml), nc=10)
    np.savez_compressed(os.path.join(OUT, 'adapt_model_str.npz'), meta=json.dumps(_meta(model, yml, 10, 64)))


def gen_modules():
    def case(name, mod, shapes, meta, seed):
        with torch.no_grad():
            if hasattr(mod, 'w'):
                mod.w.copy_(torch.rand(mod.w.shape, generator=torch.Generator().manual_seed(seed)) + 0.5)
        G.module_case(name, mod, [G.rnd(*s, seed=seed + i) for i, s in enumerate(shapes)], meta, seed=seed,
                      list_input=True)
    torch.manual_seed(50)
    case('adaptconcat_l2', C.AdaptConcat(2, 1, 24, 40), [(2, 24, 13, 17), (2, 40, 13, 17)],
         dict(module='AdaptConcat', args=[2, 1, 24, 40]), 51)
    case('adaptconcat_l3', C.AdaptConcat(3, 1, 32, 32, 64), [(2, 32, 9, 11), (2, 32, 9, 11), (2, 64, 9, 11)],
         dict(module='AdaptConcat', args=[3, 1, 32, 32, 64]), 55)
    case('adapt_add2', C.Adapt_Add2(), [(2, 24, 13, 17)] * 2, dict(module='Adapt_Add2', args=[]), 61)
    case('adapt_add3', C.Adapt_Add3(16, 16, 32), [(2, 16, 9, 11), (2, 16, 9, 11), (2, 32, 9, 11)],
         dict(module='Adapt_Add3', args=[16, 16, 32]), 65)


if __name__ == '__main__':
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ['modules', 'model']:
        globals()[f'gen_{w}']()
