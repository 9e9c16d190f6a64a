"""Plain-torch fp32 restatement of the SPD-mix downsamplers (models/common.py:1460-1467 SM, 1469-1475 MP, 1508-1521
DMMConv2, 1523-1536 DMMConv, 1538-1547 DMConv) and of a Model that contains them (TEST INFRASTRUCTURE ONLY, like
tests/adapt_ref.py).  oracle.nn does not know these modules; this file builds on its Conv / C3 / C3CA / SPPF / Concat /
Detect.

Written from the formulas.  SM(x) = cat(x[::2, ::2], x[1::2, ::2], x[::2, 1::2], x[1::2, 1::2]) over the two spatial
axes, MP = max_pool2d(2, 2); DMConv = SM(conv3x3(x)), DMMConv = cat(SM(conv3x3(x)), conv1x1(MP(x))), DMMConv2 =
cat(SM(x), conv1x1(MP(x))), every conv a Conv (conv -> BN -> SiLU).  Parameter names follow the reference's state_dict
layout (cv1.conv.weight, cv1.bn.*, cv2.*), so a reference state_dict loads unchanged.

The model fixtures carry no weights: both sides fill theirs with adapt_ref.fill_state_dict.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from adapt_ref import fill_state_dict, fixture_state  # noqa: F401  (re-exported for the tests)
from oracle import nn as onn


class SM(nn.Module):
    """models/common.py:1460-1467"""

    def __init__(self, dimension=1):
        super().__init__()

    def forward(self, x):
        return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


class MP(nn.Module):
    """models/common.py:1469-1475; a module with a child `m`, so precision_emu rounds the stored pooled map"""

    def __init__(self, k=2):
        super().__init__()
        self.m = nn.MaxPool2d(kernel_size=k, stride=k)

    def forward(self, x):
        return self.m(x)


class DMConv(nn.Module):
    """models/common.py:1538-1547"""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = onn.Conv(c1, c2, 3, 1)
        self.sm = SM()

    def forward(self, x):
        return self.sm(self.cv1(x))


class DMMConv(nn.Module):
    """models/common.py:1523-1536"""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = onn.Conv(c1, c2, 1, 1)
        self.cv2 = onn.Conv(c1, c2, 3, 1)
        self.sm = SM()
        self.mp = MP()

    def forward(self, x):
        return torch.cat([self.sm(self.cv2(x)), self.cv1(self.mp(x))], 1)


class DMMConv2(nn.Module):
    """models/common.py:1508-1521"""

    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = onn.Conv(c1, c2, 1, 1)
        self.sm = SM()
        self.mp = MP()

    def forward(self, x):
        return torch.cat([self.sm(x), self.cv1(self.mp(x))], 1)


MODS = {'DMConv': DMConv, 'DMMConv': DMMConv, 'DMMConv2': DMMConv2, 'SM': SM, 'MP': MP}
_CHANNEL = ('Conv', 'C3', 'C3CA', 'SPPF')
_REPEAT = ('C3', 'C3CA')


class Model(nn.Module):
    """the YAML walk of models/yolo.py:353-478 for the modules DM.yaml / CADM.yaml / CADMM.yaml / CADMM2.yaml use; 4
    Detect levels with strides (4, 8, 16, 32)"""

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
                cls = getattr(onn, name)
            elif name == 'Concat':
                c2, cls = sum(chs[x] for x in f), onn.Concat
            elif name == 'DMMConv':  # models/yolo.py:451-454
                c2, cls, args = 5 * args[0], DMMConv, [chs[f], args[0]]
            elif name == 'DMMConv2':  # models/yolo.py:455-458
                c2, cls, args = args[0] + 4 * chs[f], DMMConv2, [chs[f], args[0]]
            elif name == 'DMConv':  # models/yolo.py:459-462
                c2, cls, args = 4 * args[0], DMConv, [chs[f], args[0]]
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


def max_pool_ref(x):
    """F.max_pool2d(2, 2) on the CPU: the value reference of the kernel tests"""
    return F.max_pool2d(x, 2, 2)
