"""Torch restatement of the IoU-family box criteria other than SIoU, from their formulas (TEST INFRASTRUCTURE ONLY).

For an [n, 4] box A (the one that carries gradients) and an [n, 4] box B, in the dtype of A (float64 in the tests):

  I  = max(0, min(Ax2, Bx2) - max(Ax1, Bx1)) * max(0, min(Ay2, By2) - max(Ay1, By1))
  U  = wA (hA + e) + wB (hB + e) - I + e                     e = 1e-7 as the reference places it
  iou  = I / U
  giou = iou - (C - U) / C,      C = cw ch + e,  cw, ch the sides of the smallest enclosing box   (Rezatofighi 2019)
  diou = iou - rho2 / c2,        rho2 = squared centre distance,  c2 = cw^2 + ch^2 + e            (Zheng 2020)
  ciou = diou - alpha v,         v = (4 / pi^2) (atan(wB / (hB + e)) - atan(wA / (hA + e)))^2,
                                 alpha = v / (v - iou + 1 + e) held constant (detached)           (Zheng 2020)

xyxy=False: rows are (x, y, w, h); xyxy=True: rows are (x1, y1, x2, y2).  torch.minimum / maximum / clamp give the tie
rules the product states (ties split the gradient, the clamp passes it at 0).
"""
import math

import torch

KINDS = ('giou', 'diou', 'ciou', 'iou')
E = 1e-7


def _corners(b, xyxy):
    if xyxy:
        return b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    hw, hh = b[:, 2] / 2, b[:, 3] / 2
    return b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh


def bbox_iou_ref(a, b, kind, xyxy=False):
    """[n] criterion `kind` of the row pairs of a and b ([n, 4] each); differentiable in a"""
    assert kind in KINDS, kind
    b = b.to(a.dtype)
    ax1, ay1, ax2, ay2 = _corners(a, xyxy)
    bx1, by1, bx2, by2 = _corners(b, xyxy)
    ix = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0)
    iy = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    inter = ix * iy
    wa, ha = ax2 - ax1, ay2 - ay1 + E
    wb, hb = bx2 - bx1, by2 - by1 + E
    union = wa * ha + wb * hb - inter + E
    iou = inter / union
    if kind == 'iou':
        return iou
    cw = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)
    ch = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    if kind == 'giou':
        hull = cw * ch + E
        return iou - (hull - union) / hull
    diag2 = cw * cw + ch * ch + E
    dx, dy = (bx1 + bx2) - (ax1 + ax2), (by1 + by2) - (ay1 + ay2)  # twice the centre offsets
    diou = iou - (dx * dx + dy * dy) / 4 / diag2
    if kind == 'diou':
        return diou
    v = (4 / math.pi ** 2) * (torch.atan(wb / hb) - torch.atan(wa / ha)) ** 2
    alpha = (v / (v - iou + (1 + E))).detach()
    return diou - alpha * v
