"""CPU restatement of non_max_suppression with the modes beyond the default call (TEST INFRASTRUCTURE ONLY):
apriori label rows (utils/general.py:663-670), the criterion NMS of utils/general.py:727-761 over bbox_iou
(utils/general.py:764-824) and merge-NMS (utils/general.py:712-718).

fp32 torch on the CPU, one rounding per operation (every elementwise op is its own kernel: nothing fuses).  Built on
oracle.general's conventions: xywh2xyxy, ONE stable descending score order for the max_nms cut and for the greedy
walk (the reference's unstable argsort leaves ties undefined; the stable order is the definition here), and a keep
list that stops at max_keep.  With nms_type='iou', no labels and no merge it is oracle.general.non_max_suppression.
"""
import math

import torch

from oracle.general import greedy_nms, xywh2xyxy

E = 1e-7  # where the reference's bbox_iou adds its eps
KINDS = ('iou', 'giou', 'diou', 'ciou')


def criterion(kept, later, kind):
    """the giou / diou / ciou value of general.py:764-824 (corner boxes) between ONE kept box `kept` [4], the
    formula's first box, and the `later` boxes [n, 4], its second.  From the formulas (Rezatofighi 2019, Zheng 2020),
    in the operation order that is the contract: E joins both heights, the union, the hull area and the squared hull
    diagonal; the doubled centre offset is ((Bx1 + Bx2) - Ax1) - Ax2; squares are products; / 4 is a division"""
    ax1, ay1, ax2, ay2 = kept.unbind(0)
    bx1, by1, bx2, by2 = later.unbind(1)
    ix = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0)
    iy = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    overlap = ix * iy
    wa, ha = ax2 - ax1, (ay2 - ay1) + E
    wb, hb = bx2 - bx1, (by2 - by1) + E
    joint = ((wa * ha + wb * hb) - overlap) + E
    iou = overlap / joint
    hull_w = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)  # the smallest box around both
    hull_h = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    if kind == 'giou':
        hull = hull_w * hull_h + E
        return iou - (hull - joint) / hull
    diag2 = (hull_w * hull_w + hull_h * hull_h) + E
    dx = ((bx1 + bx2) - ax1) - ax2  # twice the centre offsets
    dy = ((by1 + by2) - ay1) - ay2
    dist = ((dx * dx + dy * dy) / 4) / diag2
    if kind == 'diou':
        return iou - dist
    assert kind == 'ciou', kind
    turn = torch.atan(wb / hb) - torch.atan(wa / ha)
    v = (4 / math.pi ** 2) * (turn * turn)  # aspect-ratio term; the python double becomes fp32 once
    weight = v / ((v - iou) + (1 + E))
    return iou - (dist + v * weight)


def greedy_nms_kind(boxes, scores, iou_thres, kind, max_keep=None):
    """NMS() of general.py:727-761 in the stable descending score order: the kept box is box1, a later box stays iff
    criterion <= iou_thres (so a NaN suppresses); kind 'iou' is oracle.general.greedy_nms (torchvision's test)"""
    if kind == 'iou':
        return greedy_nms(boxes, scores, iou_thres, max_keep)
    order = torch.sort(scores, stable=True, descending=True)[1]
    dead = torch.zeros(len(scores), dtype=torch.bool)
    keep = []
    for k in range(len(order)):
        i = order[k]
        if dead[i]:
            continue
        keep.append(int(i))
        if max_keep is not None and len(keep) >= max_keep:
            break
        rest = order[k + 1:]
        if len(rest):
            dead[rest[~(criterion(boxes[i], boxes[rest], kind) <= iou_thres)]] = True
    return torch.tensor(keep, dtype=torch.int64)


def box_iou(rows, cols):
    """the plain pairwise IoU of utils/metrics.py:254-276: [k, 4] x [n, 4] -> [k, n], overlap / (area_row + area_col -
    overlap), no eps"""
    def area(t):
        return (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    lo = torch.maximum(rows[:, None, :2], cols[None, :, :2])
    hi = torch.minimum(rows[:, None, 2:], cols[None, :, 2:])
    side = (hi - lo).clamp(min=0)
    overlap = side[..., 0] * side[..., 1]
    return overlap / (area(rows)[:, None] + area(cols)[None, :] - overlap)


def candidates(prediction, conf_thres=0.25, classes=None, multi_label=False, labels=()):
    """general.py:658-703 per image: the [n, 6] candidate rows (xyxy, conf, cls) in row order, before any cut"""
    nc = prediction.shape[2] - 5
    multi_label &= nc > 1
    out = []
    for b in range(prediction.shape[0]):
        x = prediction[b][prediction[b, :, 4] > conf_thres].clone()
        if labels is not None and len(labels) and len(labels[b]):
            # apriori rows after the surviving predictions: the label's xywh, objectness 1, its class one-hot
            lab = labels[b].float()
            onehot = torch.nn.functional.one_hot(lab[:, 0].long(), nc).float()
            x = torch.cat((x, torch.cat((lab[:, 1:5], torch.ones(len(lab), 1), onehot), 1)), 0)
        if not x.shape[0]:
            out.append(torch.zeros((0, 6)))
            continue
        x[:, 5:] *= x[:, 4:5]
        box = xywh2xyxy(x[:, :4])
        if multi_label:
            i, j = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).T
            x = torch.cat((box[i], x[i, j + 5, None], j[:, None].float()), 1)
        else:
            conf, j = x[:, 5:].max(1, keepdim=True)
            x = torch.cat((box, conf, j.float()), 1)[conf.view(-1) > conf_thres]
        if classes is not None:
            x = x[(x[:, 5:6] == torch.tensor(classes)).any(1)]
        out.append(x)
    return out


def merge_weights(x, keep, iou_thres, agnostic=False):
    """general.py:714-715: (hit [k, n] bool, weights [k, n] fp32) of the kept rows over all n candidates"""
    boxes = x[:, :4] + x[:, 5:6] * (0 if agnostic else 4096)
    hit = box_iou(boxes[keep], boxes) > iou_thres
    return hit, hit * x[None, :, 4]


def _two_sum(a, b):
    """a + b = s + e exactly (Knuth), all fp32"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    """a = hi + lo with 12-bit halves (Dekker / Veltkamp, fp32: 2^12 + 1)"""
    c = a * 4097.0
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    """a * b = p + e exactly, without an FMA (Dekker), all fp32"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def _dot2(w, X):
    """sum_j w[:, j] X[j, :] as an unevaluated fp32 pair (s, c): every product and every addition hands its rounding
    error on (Ogita, Rump, Oishi: Dot2), so s + c is the exact sum up to O(n 2^-48) relative"""
    s = torch.zeros(w.shape[0], X.shape[1])
    c = torch.zeros_like(s)
    for j in range(w.shape[1]):
        p, e = _two_prod(w[:, j:j + 1], X[j][None, :])
        s, q = _two_sum(s, p)
        c = c + (q + e)
    return s, c


def merged_boxes(x, weights, dtype=torch.float32):
    """general.py:716: weights [k, n] x un-offset xyxy [n, 4] / row sums.  fp64: torch.mm and the division as they
    stand, the yardstick.  fp32: the device kernel's contract -- the exact quotient rounded to fp32 once -- in fp32
    operations alone: both sums compensated (_dot2) and the quotient corrected by its exactly computed remainder, so
    the error is one fp32 rounding plus O(n 2^-48) for every n; a row that only hits itself gives (w x) / w = x.
    (A plain fp32 torch.mm followed by the division rounds up to 2 n times: 2 * 2^-24 already at n = 1.)"""
    if dtype == torch.float64:
        w = weights.to(dtype)
        return torch.mm(w, x[:, :4].to(dtype)) / w.sum(1, keepdim=True)
    assert dtype == torch.float32
    w = weights.float()
    s, c = _dot2(w, x[:, :4].float())
    S, C = _dot2(w, torch.ones(w.shape[1], 1))
    q = s / S
    ph, pl = _two_prod(q, S)
    r = (((s - ph) - pl) + c) - q * C  # (s + c) - q (S + C): s - ph is exact, the two are within a rounding
    return q + r / S


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                        multi_label=False, labels=(), max_det=300, merge=False, redundant=True, nms_type='iou',
                        merge_dtype=torch.float32):
    """utils/general.py:633-761 with labels, merge / redundant and the suppression criterion.  merge_dtype: the
    arithmetic of the merged boxes (merged_boxes: fp32 operations that round the exact quotient once; fp64 is the
    yardstick of the device kernel, whose result is then rounded to fp32 once)"""
    kind = nms_type.lower()
    assert kind in KINDS, nms_type
    max_wh, max_nms = 4096, 30000
    out = [torch.zeros((0, 6))] * prediction.shape[0]
    for b, x in enumerate(candidates(prediction, conf_thres, classes, multi_label, labels)):
        n = x.shape[0]
        if not n:
            continue
        if n > max_nms:
            x = x[torch.sort(x[:, 4], stable=True, descending=True)[1][:max_nms]]
        c = x[:, 5:6] * (0 if agnostic else max_wh)
        keep = greedy_nms_kind(x[:, :4] + c, x[:, 4], iou_thres, kind, max_det)[:max_det]
        if merge and 1 < n < 3000:
            hit, weights = merge_weights(x, keep, iou_thres, agnostic)
            x = x.clone()
            x[keep, :4] = merged_boxes(x, weights, merge_dtype).float()
            if redundant:
                keep = keep[hit.sum(1) > 1]
        out[b] = x[keep]
    return out


def cluster_prediction(seed, nimg=2, clusters=12, per=16, nc=3, second=False):
    """the crowded scene of the mode tests: per image `clusters` clusters of `per` boxes, centres uniform in
    [20, 620]^2 jittered by N(0, 6 px), sizes 12-72 px jittered by +-15 %, nc classes (one per cluster), distinct
    scores in (0.3, 0.99): prediction [nimg, clusters * per, 5 + nc] with obj = 1 and the class probability = score.
    second: every third row also carries 0.9 * score on the next class, so that multi_label has rows with two
    candidates"""
    g = torch.Generator().manual_seed(seed)
    A = clusters * per
    pred = torch.zeros(nimg, A, 5 + nc)
    for b in range(nimg):
        cxy = torch.rand(clusters, 2, generator=g) * 600 + 20
        size = torch.rand(clusters, 2, generator=g) * 60 + 12
        cls = torch.randint(0, nc, (clusters,), generator=g)
        xy = cxy[:, None, :] + torch.randn(clusters, per, 2, generator=g) * 6
        wh = size[:, None, :] * (1 + (torch.rand(clusters, per, 2, generator=g) * 2 - 1) * 0.15)
        score = (0.3 + 0.69 * (torch.randperm(A, generator=g).float() + 0.5) / A)
        pred[b, :, :2] = xy.reshape(A, 2)
        pred[b, :, 2:4] = wh.reshape(A, 2)
        pred[b, :, 4] = 1.0
        rc = cls.repeat_interleave(per)
        pred[b, torch.arange(A), 5 + rc] = score
        if second:
            r = torch.arange(0, A, 3)
            pred[b, r, 5 + (rc[r] + 1) % nc] = 0.9 * score[r]
    return pred
