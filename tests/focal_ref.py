"""Torch restatement of ComputeLoss with the FocalLoss wrapper (utils/loss.py:35-62, fl_gamma > 0) and autobalance
(utils/loss.py:207-212), built on oracle.loss.build_targets / siou (TEST INFRASTRUCTURE ONLY).

Runs in the dtype of p (float32 or float64) with autograd; target assignment is always the fp32 one, as in the product.
Two places differ from a literal transcription, both where the reference itself gives no usable number:
  * (1 - p_t) is clamped at the dtype's smallest normal before the power, so that gamma < 1 has a finite gradient where
    the sigmoid has saturated onto the target (the reference returns NaN there; for gamma >= 1 nothing changes: the
    clamped element contributes < 1e-19 to the loss and 0 to the gradient);
  * autobalance leaves a level's balance unchanged when its objectness loss is 0 or not finite (the reference raises
    ZeroDivisionError on 0).
"""
import math

import torch
import torch.nn.functional as F

from oracle.loss import build_targets, siou

ALPHA = 0.25


def smooth_bce(eps):
    return 1.0 - 0.5 * eps, 0.5 * eps


def focal_bce(x, t, pw, gamma):
    """FocalLoss(BCEWithLogitsLoss(pos_weight=pw), gamma)(x, t), mean reduction; gamma == 0 is the plain BCE."""
    loss = F.binary_cross_entropy_with_logits(x, t, pos_weight=torch.tensor([pw], dtype=x.dtype), reduction='none')
    if gamma > 0:
        s = torch.sigmoid(x)
        p_t = t * s + (1 - t) * (1 - s)
        alpha_factor = t * ALPHA + (1 - t) * (1 - ALPHA)
        modulating_factor = (1.0 - p_t).clamp_min(torch.finfo(x.dtype).tiny) ** gamma
        loss = loss * (alpha_factor * modulating_factor)
    return loss.mean()


class FocalComputeLoss:
    """ComputeLoss(model, autobalance) for hyp['fl_gamma'] >= 0.  anchors [nl, na, 2] in grid units, stride per level."""

    def __init__(self, anchors, hyp, nc, stride=(8, 16, 32), autobalance=False):
        self.anchors, self.hyp, self.nc = anchors.float(), hyp, nc
        self.gamma = float(hyp.get('fl_gamma', 0.0))
        self.cp, self.cn = smooth_bce(hyp.get('label_smoothing', 0.0))
        nl = anchors.shape[0]
        self.balance = list({3: [4.0, 1.0, 0.4]}.get(nl, [4.0, 1.0, 0.25, 0.06, 0.02]))
        self.autobalance = autobalance
        self.ssi = [float(s) for s in stride].index(16.0) if autobalance else 0

    def __call__(self, p, targets):
        h, dt = self.hyp, p[0].dtype
        tg = build_targets([x.shape for x in p], targets.float(), self.anchors, h['anchor_t'])
        lbox, lobj, lcls = (torch.zeros(1, dtype=dt) for _ in range(3))
        for i, pi in enumerate(p):
            r = tg[i]
            tobj = torch.zeros(pi.shape[:4], dtype=dt)
            n = r['b'].numel()
            if n:
                ps = pi[r['b'], r['a'], r['gj'], r['gi']]
                pxy = ps[:, :2].sigmoid() * 2 - 0.5
                pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * r['anch'].to(dt)
                iou = siou(torch.cat([pxy, pwh], 1), r['tbox'].to(dt))
                lbox = lbox + (1.0 - iou).mean()
                flat = ((r['b'] * pi.shape[1] + r['a']) * pi.shape[2] + r['gj']) * pi.shape[3] + r['gi']
                tobj.view(-1).scatter_reduce_(0, flat, iou.detach().clamp(0), reduce='amax', include_self=True)
                if self.nc > 1:
                    t = torch.full_like(ps[:, 5:], self.cn)
                    t[torch.arange(n), r['tcls']] = self.cp
                    lcls = lcls + focal_bce(ps[:, 5:], t, h['cls_pw'], self.gamma)
            obji = focal_bce(pi[..., 4], tobj, h['obj_pw'], self.gamma)
            lobj = lobj + obji * self.balance[i]
            if self.autobalance:
                o = obji.detach().item()
                if o != 0 and math.isfinite(o):
                    self.balance[i] = self.balance[i] * 0.9999 + 0.0001 / o
        if self.autobalance:
            self.balance = [x / self.balance[self.ssi] for x in self.balance]
        lbox = lbox * h['box']
        lobj = lobj * h['obj']
        lcls = lcls * h['cls']
        bs = p[0].shape[0]
        return (lbox + lobj + lcls) * bs, torch.cat([lbox, lobj, lcls]).detach()
