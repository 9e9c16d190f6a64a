"""Plain-torch fp32 restatement of the ConvMixer family (models/cspcm.py:25-41 ConvMix, 43-54 CSPCM) and of a Model that
contains it (TEST INFRASTRUCTURE ONLY, like tests/hor_ref.py).  oracle.nn does not know these modules; this file builds
on its Conv / C3 / SPPF / Concat / Detect.

Written from the formulas:
  ConvMix: x = x + BN(gelu(dw9x9(x) + b)); out = BN(gelu(conv1x1(x) + b)) -- the activation BEFORE the BatchNorm, the
           batch statistics over gelu(.), both convs biased, the depthwise one with 'same' padding (4)
  CSPCM:   cv3(cat(m(cv1(x)), cv2(x))) with m = n ConvMix(c_, c_), c_ = int(c2 * e); cv1 / cv2 / cv3 are Conv 1x1
Parameter names follow the reference's state_dict layout, so a reference state_dict loads unchanged.
"""
import copy

import torch
import torch.nn as nn

from adapt_ref import fill_state_dict  # noqa: F401  (re-exported for the tests)
from oracle import nn as onn


def _stage(dim, k, groups):
    return nn.Sequential(nn.Conv2d(dim, dim, k, padding=k // 2, groups=groups), nn.GELU(), nn.BatchNorm2d(dim))


class ConvMix(nn.Module):
    """models/cspcm.py:25-41; dim1 is unused there too"""

    def __init__(self, dim, dim1, kernel_size=9):
        super().__init__()
        self.Resnet = _stage(dim, kernel_size, dim)
        self.Conv_1x1 = _stage(dim, 1, 1)

    def forward(self, x):
        return self.Conv_1x1(x + self.Resnet(x))


class CSPCM(nn.Module):
    """models/cspcm.py:43-54"""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = onn.Conv(c1, c_, 1, 1)
        self.cv2 = onn.Conv(c1, c_, 1, 1)
        self.cv3 = onn.Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*[ConvMix(c_, c_) for _ in range(n)])

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class SpaceToDepth(nn.Module):
    """models/common.py space_to_depth: the four pixel phases stacked along the channels"""

    def __init__(self, dimension=1):
        super().__init__()

    def forward(self, x):
        return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


MODS = {'ConvMix': ConvMix, 'CSPCM': CSPCM, 'space_to_depth': SpaceToDepth}
_CHANNEL = ('Conv', 'C3', 'SPPF', 'ConvMix', 'CSPCM')
_REPEAT = ('C3',)  # models/yolo.py:399 -- CSPCM and ConvMix are NOT there: number > 1 repeats the module


class Model(nn.Module):
    """the YAML walk of models/yolo.py:353-478 for Conv / C3 / SPPF / space_to_depth / ConvMix / CSPCM / Concat /
    nn.Upsample / Detect; the Detect strides are the last of (4, 8, 16, 32)"""

    def __init__(self, cfg, ch=3, nc=None):
        super().__init__()
        d = copy.deepcopy(cfg)
        if nc:
            d['nc'] = nc
        anchors, nc, gd, gw = d['anchors'], d['nc'], d['depth_multiple'], d['width_multiple']
        na = (len(anchors[0]) // 2) if isinstance(anchors, list) else anchors
        no = na * (nc + 5)
        layers, self.save, chs, c2 = [], [], [ch], ch
        for i, (f, n, name, args) in enumerate(d['backbone'] + d['head']):
            args = [{'nc': nc, 'anchors': anchors, 'None': None, 'False': False, 'True': True}.get(a, a)
                    if isinstance(a, str) else a for a in args]
            n = max(round(n * gd), 1) if n > 1 else n
            if name in _CHANNEL:
                c1, c2 = chs[f], args[0]
                if c2 != no:
                    c2 = onn.make_divisible(c2 * gw, 8)
                args = [c1, c2, *args[1:]]
                if name in _REPEAT:
                    args.insert(2, n)
                    n = 1
                cls = MODS[name] if name in MODS else getattr(onn, name)
            elif name == 'space_to_depth':
                c2, cls = 4 * chs[f], SpaceToDepth
            elif name == 'Concat':
                c2, cls = sum(chs[x] for x in f), onn.Concat
            elif name == 'nn.Upsample':
                c2, cls = chs[f], nn.Upsample
            elif name == 'Detect':
                args.append([chs[x] for x in f])
                if isinstance(args[1], int):
                    args[1] = [list(range(args[1] * 2))] * len(f)
                cls = onn.Detect
            else:
                raise NotImplementedError(name)
            mod = nn.Sequential(*[cls(*args) for _ in range(n)]) if n > 1 else cls(*args)
            mod.i, mod.f = i, f
            self.save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
            layers.append(mod)
            if i == 0:
                chs = []
            chs.append(c2)
        self.model = nn.Sequential(*layers)
        det = self.model[-1]
        det.stride = torch.tensor((4., 8., 16., 32.)[-det.nl:])
        self.stride = det.stride

    def forward(self, x):
        ys = []
        for m in self.model:
            if m.f != -1:
                x = ys[m.f] if isinstance(m.f, int) else [x if j == -1 else ys[j] for j in m.f]
            x = m(x)
            ys.append(x if m.i in self.save else None)
        return x


def fixture_state(model, fx):
    """a fixture's parameters and buffers: fill_state_dict plus the tensors the fixture carries under sd.* (Detect's
    anchors)"""
    fill_state_dict(model)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in fx.group('sd').items():
            sd[k].copy_(v)
    return model
