"""Plain-torch fp32 restatement of the Ghost modules (models/common.py:79-82 DWConv, 666-685 GhostConv, 687-699
GhostBottleneck, 205-210 C3Ghost) and of a Model that may contain them (TEST INFRASTRUCTURE ONLY, like
tests/focal_ref.py).  oracle.nn does not know these modules; this file builds on its Conv / C3 / SPP / Concat / Detect.

Written from the formulas: a depthwise conv is conv2d with groups == channels; GhostConv(x) = cat(y, dw5x5(y)) with
y = cv1(x); GhostBottleneck(x) = conv(x) + shortcut(x).  Parameter names follow the reference's state_dict layout, so
the golden state_dicts load unchanged.
"""
import copy
import math

import torch
import torch.nn as nn

from oracle import nn as onn


class DWConv(onn.Conv):
    def __init__(self, c1, c2, k=1, s=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act)


class GhostConv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        h = c2 // 2
        self.cv1 = onn.Conv(c1, h, k, s, None, g, act)
        self.cv2 = onn.Conv(h, h, 5, 1, None, h, act)

    def forward(self, x):
        y = self.cv1(x)
        return torch.cat([y, self.cv2(y)], 1)


class GhostBottleneck(nn.Module):
    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        h = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, h, 1, 1),
                                  DWConv(h, h, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(h, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False),
                                      onn.Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def forward(self, x):
        return self.conv(x) + self.shortcut(x)


class C3Ghost(onn.C3):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        h = int(c2 * e)
        self.m = nn.Sequential(*[GhostBottleneck(h, h) for _ in range(n)])


MODS = {'Conv': onn.Conv, 'DWConv': DWConv, 'GhostConv': GhostConv, 'GhostBottleneck': GhostBottleneck,
        'C3Ghost': C3Ghost, 'SPP': lambda c1, c2, k=(5, 9, 13): onn.SPP(c1, c2, tuple(k)), 'Concat': onn.Concat,
        'Detect': onn.Detect}
_CHANNEL = ('Conv', 'DWConv', 'GhostConv', 'GhostBottleneck', 'C3Ghost', 'SPP')


class Model(nn.Module):
    """the YAML walk of models/yolo.py:353-478 for the modules above plus nn.Upsample, strides (8, 16, 32)"""

    def __init__(self, cfg, ch=3, nc=None):
        super().__init__()
        d = copy.deepcopy(cfg)
        if nc:
            d['nc'] = nc
        anchors, nc, gd, gw = d['anchors'], d['nc'], d['depth_multiple'], d['width_multiple']
        no = (len(anchors[0]) // 2) * (nc + 5)
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
                if name == 'C3Ghost':
                    args.insert(2, n)
                    n = 1
                mk = lambda: MODS[name](*args)  # noqa: E731
            elif name == 'Concat':
                c2 = sum(chs[x] for x in f)
                mk = lambda: onn.Concat(*args)  # noqa: E731
            elif name == 'nn.Upsample':
                c2 = chs[f]
                mk = lambda: nn.Upsample(*args)  # noqa: E731
            elif name == 'Detect':
                args.append([chs[x] for x in f])
                mk = lambda: onn.Detect(*args)  # noqa: E731
            else:
                raise NotImplementedError(name)
            mod = nn.Sequential(*[mk() for _ in range(n)]) if n > 1 else mk()
            mod.i, mod.f = i, f
            self.save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
            layers.append(mod)
            if i == 0:
                chs = []
            chs.append(c2)
        self.model = nn.Sequential(*layers)
        det = self.model[-1]
        det.stride = torch.tensor((8., 16., 32.))
        self.stride = det.stride

    def forward(self, x):
        ys = []
        for m in self.model:
            if m.f != -1:
                x = ys[m.f] if isinstance(m.f, int) else [x if j == -1 else ys[j] for j in m.f]
            x = m(x)
            ys.append(x if m.i in self.save else None)
        return x
