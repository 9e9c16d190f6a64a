"""Capture the reference's bbox_iou (utils/metrics.py:192-252) for the criteria other than SIoU, and its ComputeLoss
(utils/loss.py:135-218) with the bbox_iou call of loss.py:185 carrying another keyword, on its own PyTorch-CPU path
in fp32 (in-container only, like tools/gen_golden.py, whose helpers this imports).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_iou.py
Writes into tests/golden/ (data only, none of the reference's code):

  bbox_iou_<kind>.npz   kind in giou, diou, ciou, iou; gen_siou's 256 random pairs (centres in [0, 4)^2, sides in
                        [0.05, 3.05)) with the first rows replaced by EDGE below.  Both input forms:
                          b1, b2 [256, 4] xywh,  iou [256], g [256, 4] = d sum(iou) / d b1   (x1y1x2y2=False)
                          b1x, b2x the same boxes as corners, ioux, gx                       (x1y1x2y2=True)
                        None of these criteria is singular for positive sides: every value and gradient is finite
                        (asserted here), no row is to be masked.
  loss_<case>.npz       case in ciou, giou, diou, iou, ciou_focal (fl_gamma 1.5), ciou_nc1 (one class): gen_focal's
                        shape (nc 10, img 128 -> 16^2 / 8^2 / 4^2, bs 2, synth_targets(bs, 12, nc, seed=31), hyp
                        VisDrone); meta (with iou_type), targets, anchors, p.i, loss, items, gp.i
"""
import json
import os

import numpy as np
import torch

import gen_golden as GG
from gen_golden import L, M, OUT, npy, rnd, synth_targets

FLAG = {'giou': dict(GIoU=True), 'diou': dict(DIoU=True), 'ciou': dict(CIoU=True), 'iou': {}}

# (b1, b2) in xywh; every number is a multiple of 1/4 except the slivers, so the ties hold in both input forms
EDGE = [
    ((1, 1, 1, 1), (3, 3, 1, 1)),              # disjoint in x and y: inter = 0 on the clamp
    ((1, 1, 1, 1), (3, 1.25, 1, 1.5)),         # disjoint in x only
    ((1, 1, 1, 1), (2, 1, 1, 1)),              # touching along an edge: the clamp's argument is exactly 0
    ((1, 1, 1, 1), (2, 2, 1, 1)),              # touching at a corner
    ((2, 2, 1, 1.5), (2, 2, 1, 1.5)),          # identical: every min / max ties, v = 0, rho2 = 0
    ((1.5, 2.5, 2, 0.5), (1.5, 2.5, 2, 0.5)),  # identical, wide
    ((2, 2, 0.5, 0.5), (2.25, 1.75, 2, 2)),    # box 1 nested in box 2
    ((2, 2, 3, 2.5), (1.75, 2.25, 1, 0.5)),    # box 2 nested in box 1
    ((2, 2, 1, 1), (2, 2, 2, 2)),              # nested, same centre
    ((1.5, 2, 1, 1), (2, 2, 2, 2)),            # nested, sharing the left edge
    ((1, 1, 1, 2), (1.25, 1.5, 1, 1)),         # equal widths, unequal heights
    ((2, 2, 1.5, 0.5), (2, 2.5, 1.5, 2)),      # equal widths, unequal heights, same centre x
    ((2, 2, 0.05, 2), (2.5, 2, 3, 1)),         # a 0.05-wide sliver against a 3-wide box
    ((2, 2, 3, 1), (1, 2, 0.05, 3)),           # the other way round
    ((0.25, 1, 0.05, 1), (3, 1, 3, 1)),        # sliver and 3-wide box, disjoint
    ((1, 1, 1, 2), (2, 2, 0.5, 1)),            # equal aspect ratios, different sizes
]


def corners(b):
    return torch.cat([b[:, :2] - b[:, 2:] / 2, b[:, :2] + b[:, 2:] / 2], 1)


def gen_bbox_iou():
    g = torch.Generator().manual_seed(40)  # gen_siou's pairs
    n = 256
    b1 = torch.cat([torch.rand(n, 2, generator=g) * 4, torch.rand(n, 2, generator=g) * 3 + 0.05], 1)
    b2 = torch.cat([torch.rand(n, 2, generator=g) * 4, torch.rand(n, 2, generator=g) * 3 + 0.05], 1)
    b1[:len(EDGE)] = torch.tensor([e[0] for e in EDGE], dtype=torch.float32)
    b2[:len(EDGE)] = torch.tensor([e[1] for e in EDGE], dtype=torch.float32)
    for kind, flag in FLAG.items():
        d = {}
        for sfx, xyxy, (a, b) in [('', False, (b1, b2)), ('x', True, (corners(b1), corners(b2)))]:
            ar = a.clone().requires_grad_(True)
            iou = M.bbox_iou(ar.T, b, x1y1x2y2=xyxy, **flag)
            iou.sum().backward()
            assert iou.shape == (n,) and bool(torch.isfinite(iou).all()) and bool(torch.isfinite(ar.grad).all()), kind
            d.update({f'b1{sfx}': npy(a), f'b2{sfx}': npy(b), f'iou{sfx}': npy(iou), f'g{sfx}': npy(ar.grad)})
        np.savez_compressed(os.path.join(OUT, f'bbox_iou_{kind}.npz'), **d)
        print('wrote bbox_iou', kind, float(d['iou'].min()), float(d['iou'].max()), float(np.abs(d['g']).max()))


def gen_loss_iou():
    anchors = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
    bs, img = 2, 128
    ref_bbox_iou = L.bbox_iou
    for case, kind, nc, gamma in [('ciou', 'ciou', 10, 0.0), ('giou', 'giou', 10, 0.0), ('diou', 'diou', 10, 0.0),
                                  ('iou', 'iou', 10, 0.0), ('ciou_focal', 'ciou', 10, 1.5), ('ciou_nc1', 'ciou', 1, 0.0)]:
        calls = []

        def other_keyword(box1, box2, x1y1x2y2=True, SIoU=False, **kw):  # loss.py:185 with SIoU=True dropped
            assert SIoU and not kw and not x1y1x2y2
            calls.append(kind)
            return ref_bbox_iou(box1, box2, x1y1x2y2=x1y1x2y2, **FLAG[kind])

        model, hyp = GG._focal_model('VisDrone', nc, img, gamma)
        p = [rnd(bs, 3, img // s, img // s, nc + 5, seed=30 + i) for i, s in enumerate((8, 16, 32))]
        targets = synth_targets(bs, 12, nc, seed=31)
        L.bbox_iou = other_keyword
        try:
            cl = L.ComputeLoss(model)
            assert isinstance(cl.BCEobj, L.FocalLoss) == (gamma > 0)
            pp = [x.clone().requires_grad_(True) for x in p]
            loss, items = cl(pp, targets)
            loss.backward()
        finally:
            L.bbox_iou = ref_bbox_iou
        assert len(calls) == 3, calls  # every level had targets and went through the wrapper
        assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(x.grad).all()) for x in pp)
        d = {'meta': json.dumps(dict(hyp=hyp, nc=nc, img=img, anchors=anchors, stride=[8, 16, 32], iou_type=kind)),
             'targets': npy(targets), 'anchors': npy(model.model[-1].anchors), 'loss': npy(loss), 'items': npy(items)}
        for i in range(3):
            d[f'p.{i}'] = npy(p[i])
            d[f'gp.{i}'] = npy(pp[i].grad)
        np.savez_compressed(os.path.join(OUT, f'loss_{case}.npz'), **d)
        print('wrote loss', case, float(loss), items.tolist())


if __name__ == '__main__':
    gen_bbox_iou()
    gen_loss_iou()
