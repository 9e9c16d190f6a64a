"""Inputs shared by tests/test_confusion_ref.py (CPU) and tests/test_gpu_confusion.py (GPU): the recorded goldens,
hand-built images with hand-derived matrices, and a random crowded image.  TEST INFRASTRUCTURE ONLY."""
import glob
import os

import numpy as np
import torch

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'confusion_*.npz')))

L = [0, 0, 10, 10]  # the label box most cases use; a detection [0, 0, 10, h] has IoU h / 10 with it


def det(box, conf, cls):
    return [*box, conf, cls]


def lab(cls, box):
    return [cls, *box]


# name -> (detections, labels, nc, conf, iou_thres, {(row, column): count}); row = predicted, column = true, nc = background
HAND = {
    'labels_no_detections': ([], [lab(0, L), lab(2, [20, 20, 30, 30])], 3, 0.25, 0.45, {(3, 0): 1, (3, 2): 1}),
    # no pair clears the threshold: every label is background, and with no match no detection is counted
    'all_below_iou_thres': ([det([0, 0, 10, 4], 0.9, 1), det([50, 50, 60, 60], 0.9, 2)], [lab(1, L)], 3, 0.25, 0.45,
                            {(3, 1): 1}),
    'one_pair': ([det([0, 0, 10, 8], 0.9, 2)], [lab(1, L)], 3, 0.25, 0.45, {(2, 1): 1}),
    # IoU 0.6 and 0.9 over one label: the 0.9 wins, the loser is a background column entry
    'two_detections_one_label': ([det([0, 0, 10, 6], 0.9, 1), det([0, 0, 10, 9], 0.9, 2)], [lab(0, L)], 3, 0.25, 0.45,
                                 {(2, 0): 1, (1, 3): 1}),
    # IoU 0.9 with label 0, 8/9 with label 1: the detection takes label 0, label 1 stays unmatched
    'one_detection_two_labels': ([det([0, 0, 10, 9], 0.9, 2)], [lab(0, L), lab(1, [0, 0, 10, 8])], 3, 0.25, 0.45,
                                 {(2, 0): 1, (3, 1): 1}),
    # detection 0: IoU 0.7 with label A (its best) and 0.657 with label B; detection 1 has IoU 1 with A and takes it.
    # Detection 0 is then background although it clears the threshold for B, and B stays unmatched
    'best_label_taken': ([det([0, 0, 10, 7], 0.9, 1), det([0, 0, 10, 10], 0.9, 2)],
                         [lab(0, L), lab(1, [0, 0, 10, 4.6])], 3, 0.25, 0.45, {(2, 0): 1, (1, 3): 1, (3, 1): 1}),
    # IoU exactly 0.5 at iou_thres 0.5: strict >, no match
    'iou_equals_thres': ([det([0, 0, 1, 1], 0.9, 0)], [lab(0, [0, 0, 2, 1])], 3, 0.25, 0.5, {(3, 0): 1}),
    # conf exactly self.conf: filtered out, so the IoU-0.6 detection wins and the filtered one is counted nowhere
    'conf_equals_thres': ([det([0, 0, 10, 9], 0.25, 1), det([0, 0, 10, 6], 0.9, 2)], [lab(0, L)], 3, 0.25, 0.45,
                          {(2, 0): 1}),
    # the thresholds compare in fp32: conf fp32(0.3) is not > 0.3 although it is as a double
    'conf_equals_thres_fp32': ([det([0, 0, 10, 9], 0.3, 1), det([0, 0, 10, 6], 0.9, 2)], [lab(0, L)], 3, 0.3, 0.45,
                               {(2, 0): 1}),
    # exact ties (duplicate boxes), the order of a stable sort reversed: the later label / the larger detection wins
    'tie_duplicate_labels': ([det([0, 0, 10, 9], 0.9, 2)], [lab(0, L), lab(1, L)], 3, 0.25, 0.45,
                             {(2, 1): 1, (3, 0): 1}),
    'tie_duplicate_detections': ([det([0, 0, 10, 9], 0.9, 1), det([0, 0, 10, 9], 0.9, 2)], [lab(0, L)], 3, 0.25, 0.45,
                                 {(2, 0): 1, (1, 3): 1}),
    # classes are truncated: 1.9 -> 1, 0.5 -> 0
    'classes_truncate': ([det([0, 0, 10, 9], 0.9, 1.9)], [lab(0.5, L)], 3, 0.25, 0.45, {(1, 0): 1}),
}
# classes outside [0, nc) are not stored (the reference would index outside its matrix, or wrap around on a negative
# class): the matched pairs (7 <- 0) and (1 <- 9) and the unmatched class-4 detection vanish, the class-2 one counts
OUT_OF_RANGE = ([det([0, 0, 10, 9], 0.9, 0), det([20, 20, 30, 29], 0.9, 9), det([50, 50, 60, 60], 0.9, 4),
                 det([70, 70, 80, 80], 0.9, 2), det([90, 90, 95, 95], 0.9, -3)],
                [lab(7, L), lab(1, [20, 20, 30, 30]), lab(-1, [200, 200, 210, 210])], 3, 0.25, 0.45, {(2, 3): 1})


def arrays(dets, labs):
    return np.asarray(dets, np.float32).reshape(-1, 6), np.asarray(labs, np.float32).reshape(-1, 5)


def dense(nc, cells):
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for (r, c), v in cells.items():
        m[r, c] = v
    return m


def load_golden(path):
    """-> (dets list, labs list, nc, conf, iou_thres, the reference's matrix as int64)"""
    z = np.load(path)
    do, lo = z['det_off'], z['lab_off']
    dets = [z['det'][do[i]:do[i + 1]] for i in range(len(do) - 1)]
    labs = [z['lab'][lo[i]:lo[i + 1]] for i in range(len(lo) - 1)]
    want = z['matrix']
    assert want.dtype == np.float64 and np.array_equal(want, np.round(want))
    return dets, labs, int(z['nc']), float(z['conf']), float(z['iou_thres']), want.astype(np.int64)


def crowded(seed, nd, nl, nc):
    """nl label boxes, half of them beside an earlier one, and nd detections jittered around labels: detections compete
    for labels and labels for detections; confidences spread over (0, 1), classes mostly the label's"""
    g = torch.Generator().manual_seed(seed)
    cen = torch.rand(max(nl, 1), 2, generator=g) * 300 + 40
    wh = torch.rand(max(nl, 1), 2, generator=g) * 40 + 8
    for i in range(1, nl):
        if float(torch.rand(1, generator=g)) < 0.5:
            j = int(torch.randint(0, i, (1,), generator=g))
            cen[i] = cen[j] + (torch.rand(2, generator=g) - 0.5) * wh[j] * 0.5
            wh[i] = wh[j] * (0.8 + 0.4 * torch.rand(2, generator=g))
    labels = torch.cat([torch.randint(0, nc, (nl, 1), generator=g).float(), cen[:nl] - wh[:nl] / 2,
                        cen[:nl] + wh[:nl] / 2], 1)
    pick = torch.randint(0, max(nl, 1), (nd,), generator=g)
    c = cen[pick] + torch.randn(nd, 2, generator=g) * wh[pick] * 0.12
    w = wh[pick] * (1 + 0.2 * torch.randn(nd, 2, generator=g)).clamp(0.3)
    cls = torch.where(torch.rand(nd, 1, generator=g) < 0.7, labels[pick, :1] if nl else torch.zeros(nd, 1),
                      torch.randint(0, nc, (nd, 1), generator=g).float())
    dets = torch.cat([c - w / 2, c + w / 2, torch.rand(nd, 1, generator=g), cls], 1)
    return dets.float().numpy(), labels.float().numpy()
