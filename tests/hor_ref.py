"""Plain-torch fp32 restatement of the HorNet modules (models/common.py:1318-1359 GnConv, 1364-1400 HorBlock, 1402-1427
LayerNorm, 1429-1439 C3HB) and of a Model that contains them (TEST INFRASTRUCTURE ONLY, like tests/dm_ref.py).
oracle.nn does not know these modules; this file builds on its Conv / C3 / Concat / Detect.

Written from the formulas.  With dims = [c / 16, c / 8, c / 4, c / 2, c]:
  GnConv:   (pwa | abc) = conv1x1(x) split at dims[0]; dw = dwconv7x7(abc) * s split by dims;
            y = pwa * dw[0]; y = conv1x1_i(y) * dw[i + 1] for i = 0..3; out = Conv(y)
  HorBlock: x = x + gamma1 * GnConv(LN(x)); x = x + gamma2 * fc2(gelu(fc1(LN(x)))), LN over channels with the biased
            variance and eps 1e-6, the fc layers per pixel
  C3HB:     C3 whose stack is n HorBlock(c_).
Parameter names follow the reference's state_dict layout, so a reference state_dict loads unchanged.

For tests/precision_emu.py: LayerNorm is an nn.LayerNorm (one of its leaves) that permutes to channels-last and back,
and every tensor the HIP path stores that no leaf produces -- the five gate products and the two layer-scaled residual
sums -- passes through `Stored`, an nn.AvgPool2d subclass whose forward is the identity: a leaf the emulation rounds.
"""
import copy

import torch
import torch.nn as nn

from adapt_ref import fill_state_dict  # noqa: F401  (re-exported for the tests)
from oracle import nn as onn


class Stored(nn.AvgPool2d):
    """identity marking a tensor the product writes to memory (see the module docstring); no parameters.  forward hands
    its input on untouched, so the plain fp32 run keeps the reference's memory layouts and summation orders"""

    def __init__(self):
        super().__init__(1)

    def forward(self, x):
        return x


class LayerNorm(nn.LayerNorm):
    """models/common.py:1402-1427 on an NCHW tensor: the norm over channels.  channels_first is written out as the
    reference writes it (mean, biased variance, divide by the root), channels_last is F.layer_norm on the permuted
    tensor: the same function, each in the reference's own fp32 operation order"""

    def __init__(self, normalized_shape, eps=1e-6, data_format='channels_last'):
        if data_format not in ('channels_last', 'channels_first'):
            raise NotImplementedError
        super().__init__(normalized_shape, eps=eps)
        self.data_format = data_format

    def forward(self, x):
        if self.data_format == 'channels_last':
            return super().forward(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return self.weight[:, None, None] * ((x - u) / torch.sqrt(s + self.eps)) + self.bias[:, None, None]


class GnConv(nn.Module):
    """models/common.py:1318-1359"""

    def __init__(self, c1, c2, ksize=1, stride=1, order=5, gflayer=None, h=14, w=8, s=1.0):
        super().__init__()
        assert gflayer is None
        self.order = order
        self.dims = [c1 // 2 ** i for i in range(order)][::-1]
        sd = sum(self.dims)
        self.proj_in = nn.Conv2d(c1, 2 * c1, 1)
        self.dwconv = nn.Conv2d(sd, sd, 7, padding=3, bias=True, groups=sd)
        self.proj_out = onn.Conv(c1, c2, ksize, stride)
        self.pws = nn.ModuleList([nn.Conv2d(self.dims[i], self.dims[i + 1], 1) for i in range(order - 1)])
        self.scale = s
        self.store = Stored()

    def forward(self, x):
        pwa, abc = torch.split(self.proj_in(x), (self.dims[0], sum(self.dims)), dim=1)
        dw = torch.split(self.dwconv(abc) * self.scale, self.dims, dim=1)
        y = self.store(pwa * dw[0])
        for i in range(self.order - 1):
            y = self.store(self.pws[i](y) * dw[i + 1])
        return self.proj_out(y)


class HorBlock(nn.Module):
    """models/common.py:1364-1400 (drop_path = 0)"""

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6, gnconv=GnConv):
        super().__init__()
        assert drop_path == 0.
        self.norm1 = LayerNorm(dim, eps=1e-6, data_format='channels_first')
        self.gnconv = GnConv(dim, dim)
        self.norm2 = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        on = layer_scale_init_value > 0
        self.gamma1 = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if on else None
        self.gamma2 = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if on else None
        self.store = Stored()

    def forward(self, x):
        g1 = self.gamma1.view(-1, 1, 1) if self.gamma1 is not None else 1
        x = self.store(x + g1 * self.gnconv(self.norm1(x)))
        y = self.pwconv2(self.act(self.pwconv1(self.norm2(x).permute(0, 2, 3, 1))))
        if self.gamma2 is not None:  # scaled channels-last, as the reference does: the same fp32 summation order
            y = self.gamma2 * y
        return self.store(x + y.permute(0, 3, 1, 2))


class C3HB(onn.C3):
    """models/common.py:1429-1439"""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[HorBlock(c_) for _ in range(n)])


MODS = {'GnConv': GnConv, 'HorBlock': HorBlock, 'C3HB': C3HB, 'LayerNorm': LayerNorm}
_CHANNEL = ('Conv', 'C3', 'SPPF', 'C3HB', 'HorBlock', 'GnConv')
_REPEAT = ('C3', 'C3HB')


class Model(nn.Module):
    """the YAML walk of models/yolo.py:353-478 for Conv / C3 / SPPF / C3HB / HorBlock / GnConv / Concat / nn.Upsample /
    Detect; the Detect strides are the last of (4, 8, 16, 32)"""

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
    anchors and every gamma, which fill_state_dict would draw around 0 where the fixtures want U(0.5, 1.5))"""
    fill_state_dict(model)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in fx.group('sd').items():
            sd[k].copy_(v)
    return model
