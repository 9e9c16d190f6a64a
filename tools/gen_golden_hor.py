"""Capture the reference's get_dwconv(dim, 7, True) (models/common.py:1361-1362, the depthwise conv of GnConv) on its own
PyTorch-CPU path in fp32 (in-container only, like tools/gen_golden_dm.py).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_hor.py
`gen_dw7` writes tests/golden/dw7.npz (data only, none of the reference's code): for C0 in (4, 8) -- one 16-byte vector of fp32 /
bf16 -- and the three small shapes of tests/test_gpu_dw7.py, (N, H, W, C) = (2, 5, 6, C0), (1, 7, 9, 3 C0) and
(2, 16, 20, C0), the keys '<C0>.<i>.x / w / b / dz' (inputs) and '.y / dx / dw / db' (the module's output and the
gradients of sum(y * dz)).  The test's fourth shape, (2, 40, 44, 17 C0), is not here: its x and dz alone are 3.8 MB in
fp32 at C0 = 8, over the 1 MiB a committed file may have; the test draws that case from a seeded generator.

The other generators capture GnConv / HorBlock / C3HB (models/common.py:1318-1439); name them on the command line
(`modules horblock128 model`; no argument runs those three and leaves dw7.npz alone):
  gnconv / gnconv_s2 / horblock / c3hb .npz   tools/gen_golden.py's module keys: GnConv(64, 64), GnConv(64, 128, 3, 2),
                        HorBlock(64), C3HB(64, 128, 1) in fp32 on a (2, 64, 10, 12) input, gamma1 / gamma2 ~ U(0.5, 1.5)
                        and the LayerNorm affine randomised before the capture (at the default 1e-6 the whole GnConv /
                        MLP branch is invisible in the output)
  horblock128.npz       HorBlock(128), the narrowest block bf16 storage takes, on (2, 128, 8, 10): weights by
                        tests/adapt_ref.py::fill_state_dict (not stored) with gamma* ~ U(0.5, 1.5) stored as sd.gamma*;
                        in / out / gup / gin, gp.* of the 1-D parameters, dwconv.weight and pws.*.weight, gnorm / pnames
  hor_model.npz         a reduced layer list (MODEL_YAML below) at width 1.0, nc 10, 64 px, batch 2, dm_model_*'s keys;
                        sd.* holds Detect's anchors and every gamma
  hor_model_fp32min.npz the same list at half width (GnConv / HorBlock 64 wide: fp32 storage only), meta only
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
SHAPES = [(2, 5, 6, 1), (1, 7, 9, 3), (2, 16, 20, 1)]  # (N, H, W, channel vectors)


def gen_dw7():
    d, gen = {}, torch.Generator().manual_seed(707)
    for c0 in (4, 8):
        for i, (N, H, W, cv) in enumerate(SHAPES):
            ch = cv * c0
            m = C.get_dwconv(ch, 7, True)
            with torch.no_grad():
                m.weight.copy_(torch.randn(ch, 1, 7, 7, generator=gen) / 7)
                m.bias.copy_(torch.randn(ch, generator=gen))
            x = torch.randn(N, ch, H, W, generator=gen).requires_grad_(True)
            dz = torch.randn(N, ch, H, W, generator=gen)
            y = m(x)
            (y * dz).sum().backward()
            for k, v in (('x', x), ('w', m.weight), ('b', m.bias), ('dz', dz), ('y', y), ('dx', x.grad),
                         ('dw', m.weight.grad), ('db', m.bias.grad)):
                d[f'{c0}.{i}.{k}'] = npy(v)
    meta = dict(module='get_dwconv', args=['C', 7, True], shapes=SHAPES, c0=[4, 8])
    np.savez_compressed(os.path.join(OUT, 'dw7.npz'), meta=json.dumps(meta), **d)
    print('wrote dw7', sum(v.nbytes for v in d.values()) / 1e6, 'MB')


def randomize_hor(mod, gen, norms=True):
    """gamma1 / gamma2 ~ U(0.5, 1.5) and, with `norms`, the LayerNorm affine as gen_golden.randomize_bn draws
    nn.LayerNorm's (fill_state_dict has drawn it already where the weights come from there)"""
    with torch.no_grad():
        for m in mod.modules():
            if norms and isinstance(m, C.LayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
            if isinstance(m, C.HorBlock):
                for g in (m.gamma1, m.gamma2):
                    g.copy_(torch.rand(g.shape, generator=gen) + 0.5)
    return mod


def gen_modules():
    torch.manual_seed(60)
    cases = (('gnconv', 'GnConv', [64, 64]), ('gnconv_s2', 'GnConv', [64, 128, 3, 2]), ('horblock', 'HorBlock', [64]),
             ('c3hb', 'C3HB', [64, 128, 1]))
    for i, (name, cls, args) in enumerate(cases):
        mod = randomize_hor(getattr(C, cls)(*args), torch.Generator().manual_seed(160 + i))
        G.module_case(name, mod, [G.rnd(2, 64, 10, 12, seed=61 + i)], dict(module=cls, args=args), seed=61 + i)
        path = os.path.join(OUT, f'{name}.npz')
        if os.path.getsize(path) >= 2 ** 20:
            # over the committed-file limit: the two pwconv weight gradients (half the parameters) leave, their norms
            # stay as gpnorm.<key>
            d = dict(np.load(path))
            for k in [k for k in d if k.startswith('gp.') and k.endswith(('pwconv1.weight', 'pwconv2.weight'))]:
                d['gpnorm.' + k[3:]] = np.float64(np.linalg.norm(d.pop(k).astype(np.float64)))
            np.savez_compressed(path, **d)
        print(name, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 2 ** 20


def gen_horblock128():
    gen = torch.Generator().manual_seed(128)
    mod = fill_state_dict(C.HorBlock(128))
    randomize_hor(mod, gen, norms=False)
    x = torch.randn(2, 128, 8, 10, generator=gen).requires_grad_(True)
    gup = torch.randn(2, 128, 8, 10, generator=gen)
    mod.train()
    out = mod(x)
    (out * gup).sum().backward()
    params = dict(mod.named_parameters())
    d = {'meta': json.dumps(dict(module='HorBlock', args=[128])), 'in.0': npy(x), 'out.0': npy(out), 'gup.0': npy(gup),
         'gin.0': npy(x.grad), 'sd.gamma1': npy(mod.gamma1), 'sd.gamma2': npy(mod.gamma2)}
    for k, p in params.items():
        if p.dim() == 1 or k == 'gnconv.dwconv.weight' or (k.startswith('gnconv.pws.') and k.endswith('.weight')):
            d[f'gp.{k}'] = npy(p.grad)
    d['gnorm'] = np.array([float(p.grad.norm()) for p in params.values()], dtype=np.float64)
    d['pnames'] = np.array(list(params.keys()))
    path = os.path.join(OUT, 'horblock128.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path), 'bytes')


ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
MODEL_YAML = dict(
    nc=10, depth_multiple=1.0, width_multiple=1.0, anchors=ANCHORS,
    backbone=[[-1, 1, 'Conv', [64, 6, 2, 2]],      # 0 stem, P1/2
              [-1, 1, 'Conv', [128, 3, 2]],        # 1 P2/4
              [-1, 1, 'Conv', [128, 3, 2]],        # 2 P3/8
              [-1, 2, 'C3HB', [256]],              # 3 c_ = 128, two chained HorBlocks
              [-1, 1, 'Conv', [128, 1, 1]],        # 4
              [-1, 1, 'GnConv', [256, 3, 2]],      # 5 P4/16, fed by 128 channels
              [-1, 1, 'C3HB', [256, False]],       # 6
              [-1, 1, 'Conv', [256, 3, 2]]],       # 7 P5/32
    head=[[[3, 6, 7], 1, 'Detect', ['nc', 'anchors']]])


def _meta(model, yml, nc, img):
    return dict(yaml=yml, nc=nc, img=img, stride=[float(s) for s in model.stride],
                sd_shapes={k: list(v.shape) for k, v in model.state_dict().items()})


def gen_model():
    name, yml, nc, img, bs, seed = 'hor_model', deepcopy(MODEL_YAML), 10, 64, 2, 171
    torch.manual_seed(seed)
    model = fill_state_dict(Y.Model(deepcopy(yml), nc=nc))
    randomize_hor(model, torch.Generator().manual_seed(seed + 3), norms=False)
    print(name, sum(p.numel() for p in model.parameters()) / 1e6, 'M parameters')
    assert [float(s) for s in model.stride] == [8.0, 16.0, 32.0]
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randint(0, 256, (bs, 3, img, img), generator=torch.Generator().manual_seed(seed + 2)).float() / 255
    model.train()
    outs = model(x)
    gups = [torch.randn(o.shape, generator=gen) * 0.1 for o in outs]
    sum((o * g).sum() for o, g in zip(outs, gups)).backward()
    d = {'meta': json.dumps(_meta(model, yml, nc, img)), 'in.0': npy(x)}
    for k, v in sd0.items():  # what fill_state_dict does not give: Detect's anchors in grid units, every gamma
        if k.endswith('anchors') or k.rsplit('.', 1)[-1] in ('gamma1', 'gamma2'):
            d[f'sd.{k}'] = npy(v)
    for i, (o, g) in enumerate(zip(outs, gups)):
        d[f'out.{i}'] = npy(o)
        d[f'gup.{i}'] = npy(g)
    params = dict(model.named_parameters())
    blk = next(k for k, m in model.named_modules() if isinstance(m, C.HorBlock))
    own = [k for k in params if k.startswith(blk + '.') and params[k].numel() < 4096]
    assert own and all(p.grad is not None for p in params.values())
    for k in dict.fromkeys(list(params)[:6] + list(params)[-6:] + own):
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
    yml = deepcopy(MODEL_YAML)
    yml['width_multiple'] = 0.5
    model = Y.Model(deepcopy(yml), nc=nc)
    np.savez_compressed(os.path.join(OUT, 'hor_model_fp32min.npz'), meta=json.dumps(_meta(model, yml, nc, img)))


if __name__ == '__main__':
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ['modules', 'horblock128', 'model']:
        globals()[f'gen_{w}']()
