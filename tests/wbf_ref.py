"""Host restatement of weighted boxes fusion (ensemble_boxes.weighted_boxes_fusion v1.0.9, conf_type 'avg',
allows_overflow False, the call of the reference's wbf.py:67) on the padded NMS layout.

Plain loops over Python floats: IEEE fp64, one rounding per operation, no fused multiply-add, no reordered sums.
Where the library leaves an order to numpy's unstable argsort()[::-1], the order here is the definition: records by
s descending then (model, row) ascending; outputs by score descending, then label, then cluster creation index.
"""
import numpy as np


def wbf_image(rows_per_model, W, H, weights=None, iou_thr=0.55, skip_box_thr=0.0):
    """rows_per_model: per model a [k, 6] float32 array [x1, y1, x2, y2 (pixels), score, cls] -> [n, 6] float32
    fused rows [x1, y1, x2, y2 (pixels), score, label]."""
    M = len(rows_per_model)
    w = [1.0] * M if weights is None else [float(v) for v in weights]
    W, H = float(np.float32(W)), float(np.float32(H))
    # 1. prefilter
    records = {}  # label -> [(s, t, j, box)]
    for t in range(M):
        rows = np.asarray(rows_per_model[t], dtype=np.float32).reshape(-1, 6)
        for j in range(len(rows)):
            score = float(rows[j, 4])
            if score < skip_box_thr:
                continue
            x1, y1 = float(rows[j, 0]) / W, float(rows[j, 1]) / H
            x2, y2 = float(rows[j, 2]) / W, float(rows[j, 3]) / H
            if x2 < x1:
                x1, x2 = x2, x1
            if y2 < y1:
                y1, y2 = y2, y1
            box = []
            for v in (x1, y1, x2, y2):
                if v < 0.0:
                    v = 0.0
                if v > 1.0:
                    v = 1.0
                box.append(v)
            if (box[2] - box[0]) * (box[3] - box[1]) == 0.0:
                continue
            records.setdefault(int(rows[j, 5]), []).append((score * w[t], t, j, box))
    sumw = 0.0
    for v in w:
        sumw = sumw + v
    fused = []  # (score, label, creation index, box)
    for label in sorted(records):
        # 2. order
        recs = sorted(records[label], key=lambda r: (-r[0], r[1], r[2]))
        # 3. + 4. cluster
        clusters = []  # dict(box, S, conf, n)
        for s, t, j, box in recs:
            best, bi = -1.0, -1
            areaB = (box[2] - box[0]) * (box[3] - box[1])
            for ci, c in enumerate(clusters):
                cb = c['box']
                iw = max(min(cb[2], box[2]) - max(cb[0], box[0]), 0.0)
                ih = max(min(cb[3], box[3]) - max(cb[1], box[1]), 0.0)
                inter = iw * ih
                areaA = (cb[2] - cb[0]) * (cb[3] - cb[1])
                iou = inter / (areaA + areaB - inter)
                if iou > best:  # strict: the first maximum
                    best, bi = iou, ci
            if best > iou_thr:
                c = clusters[bi]
                for q in range(4):
                    p = s * box[q]
                    c['S'][q] = c['S'][q] + p
                c['conf'] = c['conf'] + s
                c['n'] += 1
                c['box'] = [c['S'][q] / c['conf'] for q in range(4)]
            else:
                clusters.append(dict(box=list(box), S=[s * box[q] for q in range(4)], conf=s, n=1))
        # 5. score
        for ci, c in enumerate(clusters):
            n = float(c['n'])
            score = c['conf'] / n * min(n, sumw) / sumw
            fused.append((score, label, ci, c['box']))
    # 6. output
    fused.sort(key=lambda f: (-f[0], f[1], f[2]))
    out = np.zeros((len(fused), 6), np.float32)
    for i, (score, label, _, box) in enumerate(fused):
        out[i] = [np.float32(box[0] * W), np.float32(box[1] * H), np.float32(box[2] * W), np.float32(box[3] * H),
                  np.float32(score), np.float32(label)]
    return out


def wbf_padded_ref(dets, counts, wh, weights=None, iou_thr=0.55, skip_box_thr=0.0):
    """dets [M, nimg, R, 6] float32, counts [M, nimg], wh [nimg, 2] (width, height) -> list of [n, 6] float32"""
    dets, counts, wh = np.asarray(dets, np.float32), np.asarray(counts), np.asarray(wh, np.float32)
    M, nimg, R, _ = dets.shape
    return [wbf_image([dets[t, b, :min(max(int(counts[t, b]), 0), R)] for t in range(M)], wh[b, 0], wh[b, 1], weights,
                      iou_thr, skip_box_thr) for b in range(nimg)]


def weighted_boxes_fusion_ref(boxes_list, scores_list, labels_list, weights=None, iou_thr=0.55, skip_box_thr=0.0):
    """the library's one-image signature (normalised boxes): (boxes [k, 4], scores [k], labels [k]) float32"""
    rows = []
    for b, s, l in zip(boxes_list, scores_list, labels_list):
        b = np.asarray(b, np.float32).reshape(-1, 4)
        s, l = np.asarray(s, np.float32).reshape(-1), np.asarray(l, np.float32).reshape(-1)
        rows.append(np.concatenate((b, s[:, None], l[:, None]), 1))
    out = wbf_image(rows, 1.0, 1.0, weights, iou_thr, skip_box_thr)
    return out[:, :4], out[:, 4], out[:, 5]
