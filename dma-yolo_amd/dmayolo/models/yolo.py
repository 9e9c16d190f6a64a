"""Drop-in Model / parse_model / Detect (models/yolo.py:40-478) on the gfx950 kernels.

Differences from the reference that do not change results:
  * strides come from a shape-only walk of the parsed graph instead of a probe forward
    (models/yolo.py:159-170); the probe's side effect on BN running stats is not reproduced
    (parity is anchored on state_dict transfer);
  * activations are NHWC in `Model.act_dtype` (float32 parity / bfloat16 throughput).
"""
import ctypes
import math
import os
import weakref
from copy import deepcopy
from pathlib import Path
from typing import List

import torch
import torch.nn as nn

from .. import functional as Fn
from ..functional import call, ptr, stream, dcode
from .common import *  # noqa: F401,F403  (the YAML namespace)
from .common import Conv, Upsample, SCConv, GhostConv, GhostBottleneck, autopad, space_to_depth, MP, DMConv, DMMConv, DMMConv2, GnConv
from .tdetect import TDetect
from ..utils.general import make_divisible
from ..utils.torch_utils import initialize_weights, fuse_conv_and_bn, copy_attr

_CAT_PLAN = os.environ.get('DMY_CAT_PLAN', '1') == '1'  # see Model._make_cat_plan
_MODEL_SINKS = os.environ.get('DMY_MODEL_SINKS', '1') != '0'  # Model-level gradient fan-out sinks


class Detect(nn.Module):
    """models/yolo.py:40-114."""
    stride = None
    onnx_dynamic = False

    def __init__(self, nc=80, anchors=(), ch=(), inplace=True):
        super().__init__()
        self.nc = nc
        self.no = nc + 5
        self.nl = len(anchors)
        self.na = len(anchors[0]) // 2
        self.grid = [torch.zeros(1)] * self.nl
        self.anchor_grid = [torch.zeros(1)] * self.nl
        self.register_buffer('anchors', torch.tensor(anchors).float().view(self.nl, -1, 2))
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)
        self.inplace = inplace

    def forward(self, x, sinks=None):
        """sinks: None or one GradSink-or-None per level input (Model fan-out), one contribution each"""
        out = self.maps(x, sinks)
        if self.training:
            return out
        return self.decode(out), out

    def maps(self, x, sinks=None):
        """the per-level head outputs [bs, na, ny, nx, no] (views), before any decode"""
        out = []
        for i in range(self.nl):
            sk = sinks[i].expect(1) if sinks is not None and sinks[i] is not None else None
            y = Fn.conv_bn_act(x[i], self.m[i].weight, self.m[i].bias, None, 1, 0, Fn.ACT_NONE, xsink=sk)
            bs, _, ny, nx = y.shape
            # NHWC [bs, ny, nx, na*no] -> [bs, na, ny, nx, no] view (no copy)
            out.append(y.permute(0, 2, 3, 1).view(bs, ny, nx, self.na, self.no).permute(0, 3, 1, 2, 4))
        return out

    @torch.no_grad()
    def decode(self, out):
        bs = out[0].shape[0]
        total = sum(self.na * p.shape[2] * p.shape[3] for p in out)
        z = torch.empty((bs, total, self.no), dtype=torch.float32, device=out[0].device)
        off = 0
        anchors = self.anchors.float().contiguous()
        sl = getattr(self, 'stride_list', None)
        if not sl or len(sl) != len(out):  # host copy of the strides: no device sync per forward (graph-capturable)
            sl = self.stride_list = [float(v) for v in self.stride.cpu()]
        if len(out) <= 4 and len({p.dtype for p in out}) == 1:  # every level in one launch
            nl, (_, na, _, _, no) = len(out), out[0].shape
            ys = (ctypes.c_void_p * nl)(*[p.data_ptr() for p in out])
            st = (ctypes.c_long * (3 * nl))(*[v for p in out for v in (p.stride(0), p.stride(2), p.stride(3))])
            hw = (ctypes.c_int * (2 * nl))(*[v for p in out for v in (p.shape[2], p.shape[3])])
            ls = (ctypes.c_float * nl)(*sl)
            call('dmy_detect_decode_levels', dcode(out[0]), nl, ys, st, hw, ls, bs, na, no, ptr(anchors), ptr(z), total,
                 stream())
            return z
        for i, p in enumerate(out):
            _, na, ny, nx, no = p.shape
            s = p.stride()
            call('dmy_detect_decode', dcode(p), ptr(p), s[0], s[2], s[3], bs, ny, nx, na, no, sl[i],
                 ptr(anchors[i]), ptr(z), off, total, stream())
            off += na * ny * nx
        return z

    def _make_grid(self, nx=20, ny=20, i=0):
        d = self.anchors[i].device
        yv, xv = torch.meshgrid([torch.arange(ny, device=d), torch.arange(nx, device=d)], indexing='ij')
        grid = torch.stack((xv, yv), 2).expand((1, self.na, ny, nx, 2)).float()
        anchor_grid = (self.anchors[i].clone() * self.stride[i]).view((1, self.na, 1, 1, 2)).expand(
            (1, self.na, ny, nx, 2)).float()
        return grid, anchor_grid


def check_anchor_order(m):
    """utils/autoanchor.py:16-23."""
    a = m.anchors.prod(-1).view(-1)
    da = a[-1] - a[0]
    ds = m.stride[-1] - m.stride[0]
    if da.sign() != ds.sign():
        m.anchors[:] = m.anchors.flip(0)


def _out_hw(m, hw):
    """Shape-only walk used for the stride probe (models/yolo.py:159-170)."""
    if isinstance(m, nn.Sequential) and not isinstance(m[0], nn.AvgPool2d):
        for mm in m:
            hw = _out_hw(mm, hw)
        return hw
    if isinstance(m, (Conv, GhostConv)):  # DWConv is a Conv; GhostConv's map is its cv1's (cv2 is k5 s1 p2)
        c = m.conv if isinstance(m, Conv) else m.cv1.conv
        k, s, p = c.kernel_size[0], c.stride[0], c.padding[0]
        return ((hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1)
    if isinstance(m, GhostBottleneck):
        return _out_hw(m.conv[1], hw)  # the stride-2 DWConv, or the Identity placeholder
    if isinstance(m, GnConv):  # proj_in, the depthwise 7x7 and the gates keep the map; HorBlock and C3HB keep it too
        return _out_hw(m.proj_out, hw)
    if isinstance(m, SCConv):
        s = m.k4[0].stride[0]
        return ((hw[0] - 1) // s + 1, (hw[1] - 1) // s + 1)
    if isinstance(m, nn.Upsample):
        sf = m.scale_factor if isinstance(m.scale_factor, (int, float)) else m.scale_factor[0]
        return (int(hw[0] * sf), int(hw[1] * sf))
    if isinstance(m, (space_to_depth, MP, DMConv, DMMConv, DMMConv2)):  # SM is a space_to_depth
        return (hw[0] // 2, hw[1] // 2)
    return hw


TTA_SCALES = (1, 1, 0.83, 0.83, 0.67, 0.67)  # models/yolo.py:196
TTA_FLIPS = (0, 3, 0, 3, 0, 3)  # models/yolo.py:197 (None -> 0; 2 up-down, 3 left-right)


def tta_plan(h, w, gs, level_hw_fn, na=3):
    """Host plan of the augmented forward (models/yolo.py:194-209, 266-275; utils/torch_utils.py:264-274) for an
    h x w image: ([(ratio, flip, (OH, OW), (OHp, OWp), level_mask, zoff) per pass], total_rows).  The image is resized
    to OH x OW and padded to OHp x OWp (scale_img's own float arithmetic); `level_hw_fn(OHp, OWp)` gives the Detect
    levels' (ny, nx) at that size, `na` anchors each.  `level_mask` has a bit per level the pass keeps: _clip_augmented
    drops the last level's rows of the first pass and the first level's rows of the last pass; `zoff` is the pass's
    first row in the concatenated result."""
    if h % gs or w % gs:
        # the clip indices are whole levels only then (and the reference's own Concat layers need it)
        raise ValueError(f'augment=True needs an image size that is a multiple of the max stride {gs}, got {h}x{w}')
    sizes, rows = [], []
    for ratio in TTA_SCALES:
        if ratio == 1.0:
            oh, ow, ohp, owp = h, w, h, w
        else:
            oh, ow = int(h * ratio), int(w * ratio)
            ohp, owp = (math.ceil(v * ratio / gs) * gs for v in (h, w))
        sizes.append(((oh, ow), (ohp, owp)))
        rows.append([na * ny * nx for ny, nx in level_hw_fn(ohp, owp)])
    nl = len(rows[0])
    g = sum(4 ** x for x in range(nl))
    full = (1 << nl) - 1
    masks = [full] * len(TTA_SCALES)
    # _clip_augmented with e = 1: the index formulas must land on one whole level
    if (sum(rows[0]) // g) * 1 != rows[0][-1] or (sum(rows[-1]) // g) * 4 ** (nl - 1) != rows[-1][0]:
        raise ValueError(f'augment=True: the clipped tails are not whole Detect levels at {h}x{w}')
    masks[0] &= ~(1 << (nl - 1))
    masks[-1] &= ~1
    passes, zoff = [], 0
    for ratio, flip, (s, sp), r, mask in zip(TTA_SCALES, TTA_FLIPS, sizes, rows, masks):
        passes.append((ratio, flip, s, sp, mask, zoff))
        zoff += sum(v for l, v in enumerate(r) if (mask >> l) & 1)
    return passes, zoff


class Model(nn.Module):
    """models/yolo.py:117-350."""

    def __init__(self, cfg='yolov5s.yaml', ch=3, nc=None, anchors=None, act_dtype=torch.float32):
        super().__init__()
        if isinstance(cfg, dict):
            self.yaml = deepcopy(cfg)
        else:
            import yaml
            self.yaml_file = Path(cfg).name
            with open(cfg, errors='ignore') as f:
                self.yaml = yaml.safe_load(f)
        ch = self.yaml['ch'] = self.yaml.get('ch', ch)
        if nc and nc != self.yaml['nc']:
            self.yaml['nc'] = nc
        if anchors:
            self.yaml['anchors'] = round(anchors)
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=[ch])
        self.names = [str(i) for i in range(self.yaml['nc'])]
        self.inplace = self.yaml.get('inplace', True)
        self.act_dtype = act_dtype
        m = self.model[-1]
        if isinstance(m, Detect):
            s = 256
            m.inplace = self.inplace
            hw = self._probe_hw(s)
            m.stride = torch.tensor([s / h for h, _ in hw], dtype=torch.float32)
            m.anchors /= m.stride.view(-1, 1, 1)
            check_anchor_order(m)
            self.stride = m.stride
            self._initialize_biases()
        elif isinstance(m, TDetect):  # models/yolo.py:173-180
            s = 256
            m.inplace = self.inplace
            hw = self._probe_hw(s)
            m.stride = torch.tensor([s / h for h, _ in hw], dtype=torch.float32)
            self.stride = m.stride
            m.bias_init()
        initialize_weights(self)

    def _probe_hw(self, s):
        """the Detect inputs' (H, W) for an s x s image (or an (h, w) pair), from the layers' shapes alone"""
        ys, hw = [], (tuple(s) if isinstance(s, (tuple, list)) else (s, s))
        for m in self.model:
            if m.f != -1:
                hw = ys[m.f] if isinstance(m.f, int) else [hw if j == -1 else ys[j] for j in m.f]
            if isinstance(m, (Detect, TDetect)):
                return hw
            if isinstance(hw, list):
                hw = hw[0]
            hw = _out_hw(m, hw)
            ys.append(hw)
        raise AssertionError('no Detect layer')

    def forward(self, x, augment=False, profile=False, visualize=False):
        if augment:
            if torch.jit.is_tracing():
                raise NotImplementedError('augment=True cannot be traced (the traced forward is one plain-path op)')
            return self._forward_augment(x)
        if torch.jit.is_tracing():
            return _traced_forward(self, x)
        return self._forward_once(x)

    # ---- test-time augmentation (models/yolo.py:194-275): six passes, each input prepared by one dmy_tta_image
    # launch and each Detect output decoded, de-scaled, de-flipped and clipped by one dmy_detect_decode_tta launch
    # straight into its rows of the combined tensor
    def _tta_plan(self, h, w):
        det = self.model[-1]
        key = (h, w)
        c = getattr(self, '_tta_plans', None)
        if c is None:
            c = self._tta_plans = {}
        if key not in c:
            c[key] = tta_plan(h, w, int(max(self._stride_list())), lambda hp, wp: self._probe_hw((hp, wp)), det.na)
        return c[key]

    def _stride_list(self):
        det = self.model[-1]
        sl = getattr(det, 'stride_list', None)
        if not sl or len(sl) != det.nl:  # host copy: no device read per forward (graph-capturable)
            sl = det.stride_list = [float(v) for v in det.stride.cpu()]
        return sl

    def _tta_passes(self, x):
        """yields (plan entry, prepared input) per pass; pass 0 is the plain input, the others one launch each"""
        if x.dim() != 4 or not x.is_cuda or getattr(x, '_dmy_s2d', 0):
            raise ValueError('augment=True takes an NCHW image batch on the GPU')
        passes, _ = self._tta_plan(int(x.shape[2]), int(x.shape[3]))
        gs = int(max(self._stride_list()))
        s2d = bool(self._s2d_stem(x))
        for k, p in enumerate(passes):
            yield p, (self.to_input(x) if k == 0 else Fn.tta_image(x, self.act_dtype, p[0], p[1], gs, s2d))

    def tta_inputs(self, x):
        """the six inputs of the augmented forward (scale_img(x.flip(f) if f else x, s, gs) per pass), each prepared
        as `to_input` prepares the plain one"""
        return [xi for _, xi in self._tta_passes(x)]

    @torch.no_grad()
    def _forward_augment(self, x):
        det = self.model[-1]
        if isinstance(det, TDetect):
            raise NotImplementedError('augment=True is defined for the anchor-based Detect head only '
                                      '(_descale_pred does not fit the TDetect output)')
        if self.training:
            raise RuntimeError('augment=True is an eval-mode forward: call model.eval() first')
        bs, _, h, w = x.shape
        passes, total = self._tta_plan(int(h), int(w))
        z = torch.empty((bs, total, det.no), dtype=torch.float32, device=x.device)
        anchors = det.anchors.float().contiguous()
        sl = self._stride_list()
        nl = det.nl
        ls = (ctypes.c_float * nl)(*sl)
        for (ratio, flip, _, (hp, wp), mask, zoff), xi in self._tta_passes(x):
            out = self._forward_once(xi, raw=True)
            lhw = [(p.shape[2], p.shape[3]) for p in out]
            if lhw != [tuple(v) for v in self._probe_hw((hp, wp))] or len({p.dtype for p in out}) != 1:
                raise RuntimeError(f'augment=True: head maps {lhw} do not match the plan for a {hp}x{wp} pass')
            ys = (ctypes.c_void_p * nl)(*[p.data_ptr() for p in out])
            st = (ctypes.c_long * (3 * nl))(*[v for p in out for v in (p.stride(0), p.stride(2), p.stride(3))])
            hw = (ctypes.c_int * (2 * nl))(*[v for p in out for v in (p.shape[2], p.shape[3])])
            call('dmy_detect_decode_tta', dcode(out[0]), nl, ys, st, hw, ls, bs, det.na, det.no, ptr(anchors), ptr(z),
                 total, float(ratio), int(flip), float(h), float(w), mask, zoff, stream())
        return z, None

    def _s2d_stem(self, x):
        """layer 0 is the k6 s2 p2 stem Conv (every yolov5* / DMA-YOLO yaml) and the image allows the
        space-to-depth form (even H, W; no input gradient)"""
        m0 = self.model[0]
        if type(m0) is not Conv or x.dim() != 4 or x.requires_grad or x.shape[2] % 2 or x.shape[3] % 2:
            return False
        c = m0.conv
        return (c.kernel_size == (6, 6) and c.stride == (2, 2) and c.padding == (2, 2) and c.in_channels == x.shape[1]
                and c.groups == 1 and getattr(self, 's2d_stem', True))

    def to_input(self, x):
        """uint8/float NCHW image batch -> NHWC act_dtype (train.py:402 `/255` for uint8).  With the k6 s2 p2
        stem the image is stored space-to-depth (Fn.image_s2d) and the stem runs as a k3 s1 p1 conv."""
        if x.dtype == self.act_dtype and x.dim() == 4 and (x.shape[1] == 1 or x.stride(1) == 1):
            return x
        if x.is_cuda and self._s2d_stem(x):
            return Fn.image_s2d(x, self.act_dtype)
        y = Fn.ToNHWC.apply(x, self.act_dtype)
        y._dmy_cpad = Fn.vec_pad(x.shape[1], self.act_dtype)  # zero-padded channels
        return y

    def _weight_prep(self, dev):
        """functional.WeightPrep over every groups-1 or depthwise Conv2d except a 3-channel stem (space-to-depth /
        channel-padded, prepped by its own layout kernel); rebuilt when the parameters move or fuse() ran"""
        first = next(self.parameters())
        key = (first.data_ptr(), dev, self.act_dtype)
        c = getattr(self, '_prep', None)
        if c is None or c[0] != key:
            ws = [m.weight for m in self.modules() if isinstance(m, nn.Conv2d) and
                  (m.groups == 1 or m.groups == m.in_channels == m.out_channels) and m.in_channels > 4 and
                  m.dilation in (1, (1, 1)) and m.weight.requires_grad]
            c = self._prep = (key, Fn.WeightPrep(ws, self.act_dtype, dev))
        return c[1]

    def _wgrad_arena(self):
        """Fresh zeroed weight-gradient arena for this training forward (functional.WgradArena)."""
        lay = getattr(self, '_arena_layout', None)
        first = next(self.parameters())
        if lay is None or lay[0] != (first.data_ptr(), first.device):
            offs, n = Fn.WgradArena.layout(self.parameters())
            lay = self._arena_layout = ((first.data_ptr(), first.device), offs, n)
        return Fn.WgradArena(torch.zeros(lay[2], dtype=torch.float32, device=first.device), lay[1])

    def _forward_once(self, x, profile=False, visualize=False, raw=False):
        """raw: stop before the Detect decode and return the head maps (the augmented forward decodes them itself)"""
        x = self.to_input(x)
        if self._cat_plans is None:
            self._cat_plans = {}
        y = []
        arena = self.training and torch.is_grad_enabled() and x.is_cuda
        prev = Fn.WgradArena.current, Fn.WeightPrep.current
        if arena:
            Fn.WgradArena.current = self._wgrad_arena()
            self._last_arena = weakref.ref(Fn.WgradArena.current)  # ddp.ArenaDDP all-reduces slices of it
            Fn.WeightPrep.current = self._weight_prep(x.device).launch()
        fan = self._fanout() if _MODEL_SINKS and torch.is_grad_enabled() and self.training else {}
        sinks = {}
        skey = tuple(x.shape) + (x.dtype,)
        plan = self._cat_plans.get(skey) if _CAT_PLAN else None
        shapes = [] if _CAT_PLAN and plan is None else None
        bufs = {}
        try:
            for m in self.model:
                if m.f != -1:
                    x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
                kw = self._sink_kw(m, sinks) if sinks else None
                if plan is not None and m.i in plan:  # write straight into a later plain Concat's channel slice
                    c, c0, C, shp = plan[m.i]
                    if c not in bufs:
                        bufs[c] = Fn.concat_buffer(*shp, x if torch.is_tensor(x) else x[0])
                    kw = dict(kw or {}, out=bufs[c][:, c0:c0 + C])
                if raw and m is self.model[-1]:
                    x = m.maps(x)
                else:
                    x = m(x, **kw) if kw else m(x)
                y.append(x if m.i in self.save else None)
                if shapes is not None:
                    shapes.append(tuple(x.shape) if torch.is_tensor(x) else None)
                if m.i in fan:
                    sinks[m.i] = Fn.GradSink(0)
        finally:
            Fn.WgradArena.current, Fn.WeightPrep.current = prev
        if shapes is not None:
            self._cat_plans[skey] = self._make_cat_plan(shapes)
        return x

    # In-place plain Concat across layers (DMY_CAT_PLAN=0 turns it off): after a first forward at an input shape has
    # recorded every layer's output shape, each later forward at that shape allocates every plain Concat's buffer
    # ahead and hands its producers (Conv, C3, Upsample: the modules whose forward takes out=) their channel slice,
    # so ConcatFn recognises the in-place slices and copies nothing (yolov5s's head: 8 slice copies per forward).
    # The producers' other consumers read the slice through its pixel stride.  Only concats whose every input comes
    # from such a producer, each feeding no other concat.
    _cat_plans = None

    def _make_cat_plan(self, shapes):
        import inspect
        takes_out = lambda m: 'out' in inspect.signature(m.forward).parameters  # noqa: E731
        users = {}
        for m in self.model:
            if type(m).__name__ == 'Concat':
                for j in ([m.f] if isinstance(m.f, int) else m.f):
                    users.setdefault(m.i - 1 if j == -1 else j, []).append(m.i)
        plan = {}
        for m in self.model:
            if type(m).__name__ != 'Concat' or isinstance(m.f, int):
                continue
            src = [m.i - 1 if j == -1 else j for j in m.f]
            shp = [shapes[j] for j in src]
            if any(sh is None or len(sh) != 4 for sh in shp) or len(set(src)) != len(src):
                continue
            if any(len(users.get(j, [])) != 1 or not takes_out(self.model[j]) for j in src):
                continue
            if len({(sh[0], sh[2], sh[3]) for sh in shp}) != 1:
                continue
            Ct, c0 = sum(sh[1] for sh in shp), 0
            N, _, H, W = shp[0]
            for j, sh in zip(src, shp):
                plan[j] = (m.i, c0, sh[1], (N, Ct, H, W))
                c0 += sh[1]
        return plan

    # gradient fan-out: a layer output read by several layers (the BiFPN skips, the P3-P5 outputs read by a Conv and
    # Detect) gets one GradSink that the sink-aware consumers' backward kernels write / accumulate into, so autograd
    # does not sum their contributions with separate ATen add kernels (DMY_MODEL_SINKS=0 turns it off).  On by default
    # since round 6 (no ATen arithmetic on the hot path); same-box A/Bs (profiles/r02/ab_model_sinks.log,
    # profiles/r04/model_sinks_ab.log) put it within the +-0.5 % run-to-run noise -- DMA-1536 +0.35 % with Detect
    # included, -0.3 %..+0.05 % without; yolov5s -0.3 % with Detect (its only multi-consumer outputs are read by a Conv
    # and Detect, whose narrow-K data-grad then accumulates), so Detect joins only under DMY_SINK_DETECT=1.
    _SINK_TYPES = ('Conv', 'SCConv', 'AdConcat2', 'AdConcat3', 'AdaptConcat', 'Adapt_Add2', 'Adapt_Add3') + \
        (('Detect',) if os.environ.get('DMY_SINK_DETECT') == '1' else ())

    def _fanout(self):
        """{layer index: consumer count} for outputs read by >= 2 layers, >= 1 of them sink-aware (cached)"""
        if getattr(self, '_fan', None) is None:
            cons = {}
            for m in self.model:
                for j in ([m.f] if isinstance(m.f, int) else m.f):
                    cons.setdefault(m.i - 1 if j == -1 else j, []).append(type(m).__name__)
            self._fan = {i: len(c) for i, c in cons.items() if len(c) >= 2 and any(t in self._SINK_TYPES for t in c)}
        return self._fan

    def _sink_kw(self, m, sinks):
        """keyword arguments handing layer m its inputs' fan-out sinks, or None"""
        name = type(m).__name__
        if name not in self._SINK_TYPES:
            return None
        src = [m.i - 1 if j == -1 else j for j in ([m.f] if isinstance(m.f, int) else m.f)]
        sk = [sinks.get(j) for j in src]
        if all(s is None for s in sk):
            return None
        if name == 'Conv':
            return {'xsink': sk[0].expect(1)}
        if name == 'SCConv':
            return {'xsink': sk[0]}
        return {'sinks': sk}

    def _initialize_biases(self, cf=None):
        """models/yolo.py:293-301."""
        m = self.model[-1]
        for mi, s in zip(m.m, m.stride):
            b = mi.bias.view(m.na, -1)
            b.data[:, 4] += math.log(8 / (640 / s) ** 2)
            b.data[:, 5:] += math.log(0.6 / (m.nc - 0.999999)) if cf is None else torch.log(cf / cf.sum())
            mi.bias = torch.nn.Parameter(b.view(-1), requires_grad=True)

    def fuse(self):
        """models/yolo.py:315-323: BN folded into YAML-level Conv layers only."""
        for m in self.model:
            if isinstance(m, Conv) and hasattr(m, 'bn'):
                m.conv = fuse_conv_and_bn(m.conv, m.bn)
                delattr(m, 'bn')
                m.forward = m.forward_fuse
        self._prep = None
        return self

    def _apply(self, fn):
        self = super()._apply(fn)
        m = self.model[-1]
        if isinstance(m, Detect):
            m.stride_list = [float(v) for v in m.stride.cpu()] if m.stride.numel() else []
            m.stride = fn(m.stride)
            m.grid = list(map(fn, m.grid))
            if isinstance(m.anchor_grid, list):
                m.anchor_grid = list(map(fn, m.anchor_grid))
        elif isinstance(m, TDetect):  # models/yolo.py:345-348; the stride list for the kernels stays on the host
            m.stride_list = [float(v) for v in m.stride.cpu()] if m.stride.numel() else []
            m.stride = fn(m.stride)
            m.anchors = fn(m.anchors)
            m.strides = fn(m.strides)
        return self

    def autoshape(self):
        """models/yolo.py:325-329: wrap the model for raw-image inference (pre-process, forward, NMS, box rescale)."""
        from .common import AutoShape
        m = AutoShape(self)
        copy_attr(m, self, include=('yaml', 'nc', 'hyp', 'names', 'stride'), exclude=())
        return m

    def info(self, verbose=False, img_size=640):
        n_p = sum(x.numel() for x in self.parameters())
        return n_p


_CH_MODS = None


def _namespace():
    import types
    from . import common as C
    ns = {k: getattr(C, k) for k in C.__all__}
    ns['Detect'] = Detect
    ns['TDetect'] = TDetect
    ns['nn'] = types.SimpleNamespace(Upsample=Upsample, BatchNorm2d=nn.BatchNorm2d)
    return ns


def parse_model(d, ch):
    """models/yolo.py:353-478 for the hot-path module set (eval of YAML names in this namespace)."""
    from . import common as C
    ns = _namespace()
    anchors, nc, gd, gw = d['anchors'], d['nc'], d['depth_multiple'], d['width_multiple']
    na = (len(anchors[0]) // 2) if isinstance(anchors, list) else anchors
    no = na * (nc + 5)
    ev = dict(ns, nc=nc, anchors=anchors)
    chan_mods = (C.Conv, C.DWConv, C.GhostConv, C.GhostBottleneck, C.C3Ghost, C.Bottleneck, C.SPPF, C.C3, C.C3TR, C.C3STR, C.CoorAttention, C.CABottleneck, C.C3CA,
                 C.SPPFCSPC, C.SCConv, C.SPP, C.CBAM, C.C3HB, C.HorBlock, C.GnConv)
    rep_mods = (C.C3, C.C3TR, C.C3STR, C.C3CA, C.C3Ghost, C.C3HB)
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, m, args) in enumerate(d['backbone'] + d['head']):
        m = eval(m, ev) if isinstance(m, str) else m
        for j, a in enumerate(args):
            try:
                args[j] = eval(a, ev) if isinstance(a, str) else a
            except NameError:
                pass
        n = n_ = max(round(n * gd), 1) if n > 1 else n
        if m in chan_mods:
            c1, c2 = ch[f], args[0]
            if c2 != no:
                c2 = make_divisible(c2 * gw, 8)
            args = [c1, c2, *args[1:]]
            if m in rep_mods:
                args.insert(2, n)
                n = 1
        elif m is nn.BatchNorm2d:  # YAML-level; SyncBatchNorm only ever comes from converting the built model
            args = [ch[f]]
        elif m in (C.Concat, C.AdConcat2, C.AdConcat3):
            c2 = sum(ch[x] for x in f)
        elif m in (C.ConvMix, C.CSPCM):  # models/yolo.py:409-413: n is NOT inserted, so number > 1 repeats the module
            c1, c2 = ch[f], args[0]
            if c2 != no:
                c2 = make_divisible(c2 * gw, 8)
            args = [c1, c2, *args[1:]]
        elif m in (C.AdaptConcat, C.AdaptADD):  # models/yolo.py:415-419
            c2 = sum(ch[x] for x in f)
            args = [len(f), *args]
        elif m in (C.Adapt_Add2, C.Adapt_Add3):  # models/yolo.py:420-421
            c2 = max(ch[x] for x in f)
        elif m is Detect:
            args.append([ch[x] for x in f])
            if isinstance(args[1], int):
                args[1] = [list(range(args[1] * 2))] * len(f)
        elif m is TDetect:
            args.append([ch[x] for x in f])
        elif m in (space_to_depth, C.SM):
            c2 = 4 * ch[f]
        elif m is DMMConv:  # models/yolo.py:451-462: no width multiple, no make_divisible
            c1, c2, args = ch[f], 5 * args[0], [ch[f], args[0]]
        elif m is DMMConv2:
            c1, c2, args = ch[f], args[0] + 4 * ch[f], [ch[f], args[0]]
        elif m is DMConv:
            c1, c2, args = ch[f], 4 * args[0], [ch[f], args[0]]
        elif m in (Upsample, MP):
            c2 = ch[f]
        else:
            raise NotImplementedError(f'YAML module {m} is outside the DMA-YOLO hot path')
        m_ = nn.Sequential(*(m(*args) for _ in range(n))) if n > 1 else m(*args)
        t = str(m)[8:-2].replace('__main__.', '')
        np_ = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type, m_.np = i, f, t, np_
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


# ------------------------------------------------------------------ torch.jit.trace support
# The reference logs the model graph at the first batch (utils/loggers/__init__.py:86:
# tb.add_graph(torch.jit.trace(de_parallel(model), imgs[0:1], strict=False))).  The per-layer HIP launches go
# through ctypes, which the tracer cannot see, so under tracing the whole forward is ONE registered dispatcher op,
# dmayolo::model_forward (torch.library): the trace records that node (and can replay it), the op runs the
# ordinary HIP forward below the tracer.  Outputs are copies (a custom op may not return views of its
# intermediates); train mode returns the Detect maps, eval mode (decoded boxes, maps).
_TRACE_MODELS = weakref.WeakValueDictionary()


@torch.library.custom_op('dmayolo::model_forward', mutates_args=())
def _model_forward_op(x: torch.Tensor, key: int) -> List[torch.Tensor]:
    m = _TRACE_MODELS[key]
    with torch.no_grad():
        y = m._forward_once(x)
    if isinstance(y, tuple):
        return [y[0].clone()] + [o.clone() for o in y[1]]
    return [o.clone() for o in y]


def _traced_forward(model, x):
    _TRACE_MODELS[id(model)] = model
    res = torch.ops.dmayolo.model_forward(x, id(model))
    return list(res) if model.training else (res[0], list(res[1:]))
