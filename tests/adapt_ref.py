"""Plain-torch fp32 restatement of the adaptive-fusion modules (models/common.py:953-992 AdaptConcat, 1028-1044
Adapt_Add2, 1046-1061 Adapt_Add3, 1063-1081 add_conv, 1451-1458 space_to_depth) and of a Model that may contain them
(TEST INFRASTRUCTURE ONLY, like tests/ghost_ref.py).  oracle.nn does not know these modules; this file builds on its
Conv / C3 / C3CA / C3STR / SPPF / Concat / Detect.

Written from the formulas.  AdaptConcat: m_l = leaky_0.1(bn(conv1x1(x_l))) with 16 channels per level,
a = softmax_l(conv1x1_bias(cat m_l)), out = cat(x_l * a_l).  Adapt_Add: silu(sum_i w_i / (sum w + 1e-4) * x_i), the
3-input form passing x_0 and x_1 through one shared 1x1 conv with bias first.  Parameter names follow the reference's
state_dict layout, so a reference state_dict loads unchanged.

fill_state_dict() is shared with tools/gen_golden_adapt.py: the model fixtures carry no weights (a half-precision
state_dict alone is larger than the 1 MiB file limit), both sides fill theirs from the same generator keyed by
tensor name and shape.
"""
import copy
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nn as onn


def add_conv(cin, cout, k=1, s=1):
    """models/common.py:1063-1081"""
    st = nn.Sequential()
    st.add_module('conv', nn.Conv2d(cin, cout, k, s, (k - 1) // 2, bias=False))
    st.add_module('batch_norm', nn.BatchNorm2d(cout))
    st.add_module('leaky', nn.LeakyReLU(0.1))
    return st


class AdaptConcat(nn.Module):
    """models/common.py:953-992"""

    def __init__(self, level, dimension, dim1, dim2, dim3=1, rfb=False):
        super().__init__()
        self.level = level
        cc = 8 if rfb else 16
        for i, d in enumerate((dim1, dim2, dim3)):  # :963-965: three maps whatever the level
            setattr(self, f'weight_map{i}', add_conv(d, cc, 1, 1))
        self.weight_levels = nn.Conv2d(cc * level, level, 1)

    def forward(self, x):
        maps = [getattr(self, f'weight_map{i}')(x[i]) for i in range(self.level)]
        a = F.softmax(self.weight_levels(torch.cat(maps, 1)), dim=1)
        return torch.cat([x[i] * a[:, i:i + 1] for i in range(self.level)], 1)


def _norm(w):
    return w / (w.sum() + 1e-4)


class Adapt_Add2(nn.Module):
    """models/common.py:1028-1044"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(2))
        self.silu = nn.SiLU()  # a module as in the reference (:1038), so precision_emu rounds the stored output

    def forward(self, x):
        wn = _norm(self.w)
        return self.silu(wn[0] * x[0] + wn[1] * x[1])


class Adapt_Add3(nn.Module):
    """models/common.py:1046-1061"""

    def __init__(self, d1, d2, d3):
        super().__init__()
        self.w = nn.Parameter(torch.ones(3))
        self.conv = nn.Conv2d(d1, d3, 1)
        self.silu = nn.SiLU()

    def forward(self, x):
        wn = _norm(self.w)
        return self.silu(wn[0] * self.conv(x[0]) + wn[1] * self.conv(x[1]) + wn[2] * x[2])


class space_to_depth(nn.Module):
    """models/common.py:1451-1458"""

    def __init__(self, dimension=1):
        super().__init__()

    def forward(self, x):
        return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


MODS = {'AdaptConcat': AdaptConcat, 'Adapt_Add2': Adapt_Add2, 'Adapt_Add3': Adapt_Add3}
_CHANNEL = ('Conv', 'C3', 'C3CA', 'C3STR', 'SPPF')
_REPEAT = ('C3', 'C3CA', 'C3STR')


class Model(nn.Module):
    """the YAML walk of models/yolo.py:353-478 for the modules the adaptive-fusion YAMLs use; 4 Detect levels with
    strides (4, 8, 16, 32)"""

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
            elif name == 'AdaptConcat':  # models/yolo.py:415-419
                c2, cls, args = sum(chs[x] for x in f), AdaptConcat, [len(f), *args]
            elif name in ('Adapt_Add2', 'Adapt_Add3'):  # models/yolo.py:420-421
                c2, cls = max(chs[x] for x in f), MODS[name]
            elif name == 'space_to_depth':
                c2, cls = 4 * chs[f], space_to_depth
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


def fill_state_dict(model):
    """Overwrite every floating-point tensor of model.state_dict() except Detect's anchors with values drawn from a
    numpy generator seeded by the tensor's name (crc32) -- the same values for any model with the same keys and shapes.
    Conv / linear weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2), BN and fusion weights ~ U(0.5, 1.5), running_mean ~
    N(0, 0.1^2), running_var ~ U(0.5, 1.5); anything else ~ N(0, 0.1^2)."""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if not v.dtype.is_floating_point or k.endswith(('anchors', 'anchor_grid')):
                continue
            rng = np.random.default_rng(zlib.crc32(k.encode()))
            leaf = k.rsplit('.', 1)[-1]
            if v.dim() >= 2 and leaf == 'weight':
                a = rng.standard_normal(v.shape) / np.sqrt(v[0].numel())
            elif leaf == 'running_var' or leaf == 'w' or (leaf == 'weight' and v.dim() == 1):
                a = rng.uniform(0.5, 1.5, v.shape)
            else:
                a = rng.standard_normal(v.shape) * 0.1
            v.copy_(torch.from_numpy(a.astype(np.float32)))
    return model


def fixture_state(model, fx):
    """a model fixture's parameters and buffers: fill_state_dict plus the tensors the fixture does carry (Detect's
    anchors)"""
    fill_state_dict(model)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in fx.group('sd').items():
            sd[k].copy_(v)
    return model


def run_case(fx, mod, device='cpu', dtype=torch.float32):
    """tests/test_oracle_golden.py::run_module_case for a module that takes a list of inputs: train-mode forward +
    backward and eval forward of `mod` on fixture `fx`, in check_module_case's result layout"""
    from golden_util import load_sd
    onn.bn_defaults(mod)
    load_sd(mod, fx.group('sd'))
    mod = mod.to(device)
    ins = [x.to(device, dtype) for x in fx.seq('in')]
    if device != 'cpu':
        ins = [x.contiguous(memory_format=torch.channels_last) for x in ins]
    ins = [x.requires_grad_(True) for x in ins]
    mod.train()
    out = mod(ins)
    gup = fx.seq('gup')[0].to(device, dtype)
    (out.float() * gup.float()).sum().backward()
    res = dict(out=[out.detach().float().cpu()], gin=[x.grad.float().cpu() for x in ins],
               gp={k: p.grad.float().cpu() for k, p in mod.named_parameters() if p.grad is not None},
               buf={k: v.float().cpu().clone() for k, v in mod.state_dict().items() if 'running' in k})
    load_sd(mod, fx.group('sd'))
    mod.eval()
    with torch.no_grad():
        res['eout'] = [mod([x.detach() for x in ins]).float().cpu()]
    return res
