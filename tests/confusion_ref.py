"""Numpy restatement of the confusion-matrix matching (TEST INFRASTRUCTURE ONLY: imported by tests/ only), the
expected side of tests/test_gpu_confusion.py.  Pinned against the reference's own ConfusionMatrix.process_batch
(utils/metrics.py:122-160) by tests/golden/confusion_*.npz in tests/test_confusion_ref.py.

Per image, with detections [N, 6] (x1 y1 x2 y2 conf cls) and labels [M, 5] (cls x1 y1 x2 y2), all fp32:
  * only detections with conf > conf_thres take part;
  * (label l, detection d) is a candidate when iou(l, d) > iou_thres, whatever the classes;
  * every detection keeps its highest-IoU candidate label (exact tie: the larger label index);
  * among these survivors every label keeps its highest-IoU detection (exact tie: the larger detection index);
  * matched label of class gc: matrix[cls(d), gc] += 1; unmatched label: matrix[nc, gc] += 1;
  * if the image has at least one match, every filtered detection that won no label: matrix[cls(d), nc] += 1.
The thresholds compare in fp32 (a Python scalar against an fp32 tensor is rounded to fp32 first), classes are the
float columns truncated towards zero, and an update whose class falls outside [0, nc) is dropped.
The tie rules are the order numpy gives the reference for 16 or fewer candidates (a stable sort, reversed).
"""
import numpy as np


def box_iou(lab_xyxy, det_xyxy):
    """[M, 4] x [N, 4] -> [M, N] fp32, no eps: every operation rounds once in fp32 (utils/metrics.py:254-276)."""
    a = np.asarray(lab_xyxy, np.float32)[:, None, :]
    b = np.asarray(det_xyxy, np.float32)[None, :, :]
    zero = np.float32(0)
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), zero)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), zero)
    inter = w * h
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    with np.errstate(invalid='ignore', divide='ignore'):
        return (inter / (area_a + area_b - inter)).astype(np.float32)


def match(det, lab, conf_thres, iou_thres):
    """-> (kept: indices of the detections that pass the confidence filter, lab_det [M]: every label's winning
    detection (an index into det) or -1)."""
    det = np.asarray(det, np.float32).reshape(-1, 6)
    lab = np.asarray(lab, np.float32).reshape(-1, 5)
    kept = np.flatnonzero(det[:, 4] > np.float32(conf_thres))
    iou = box_iou(lab[:, 1:], det[kept, :4])
    best_lab = {}  # detection -> (iou, label)
    for k, d in enumerate(kept):
        for l in range(lab.shape[0]):
            v = iou[l, k]
            if v > np.float32(iou_thres) and (d not in best_lab or v >= best_lab[d][0]):
                best_lab[d] = (v, l)
    lab_det = np.full(lab.shape[0], -1, np.int64)
    lab_iou = np.zeros(lab.shape[0], np.float32)
    for d in sorted(best_lab):
        v, l = best_lab[d]
        if lab_det[l] < 0 or v >= lab_iou[l]:
            lab_det[l], lab_iou[l] = d, v
    return kept, lab_det


def update(matrix, det, lab, conf_thres=0.25, iou_thres=0.45):
    """adds one image into matrix [(nc + 1), (nc + 1)] int64 in place and returns it"""
    nc = matrix.shape[0] - 1
    det = np.asarray(det, np.float32).reshape(-1, 6)
    lab = np.asarray(lab, np.float32).reshape(-1, 5)
    kept, lab_det = match(det, lab, conf_thres, iou_thres)
    dcls = np.trunc(det[:, 5]).astype(np.int64)
    gcls = np.trunc(lab[:, 0]).astype(np.int64)

    def add(row, col):
        if 0 <= row <= nc and 0 <= col <= nc:
            matrix[row, col] += 1

    for l, d in enumerate(lab_det):
        if not 0 <= gcls[l] < nc:
            continue
        if d >= 0:
            if 0 <= dcls[d] < nc:
                add(dcls[d], gcls[l])
        else:
            add(nc, gcls[l])
    if (lab_det >= 0).any():
        winners = set(lab_det[lab_det >= 0].tolist())
        for d in kept:
            if d not in winners and 0 <= dcls[d] < nc:
                add(dcls[d], nc)
    return matrix


def confusion_matrix(dets, labs, nc, conf_thres=0.25, iou_thres=0.45):
    """lists of per-image detections / labels -> the [(nc + 1), (nc + 1)] int64 matrix"""
    matrix = np.zeros((nc + 1, nc + 1), np.int64)
    for det, lab in zip(dets, labs):
        update(matrix, det, lab, conf_thres, iou_thres)
    return matrix


def distinct_ious(det, lab, conf_thres, iou_thres):
    """the fixtures' condition: within the image all IoUs above the threshold are pairwise distinct in fp32"""
    det = np.asarray(det, np.float32).reshape(-1, 6)
    lab = np.asarray(lab, np.float32).reshape(-1, 5)
    kept = det[det[:, 4] > np.float32(conf_thres)]
    iou = box_iou(lab[:, 1:], kept[:, :4])
    v = iou[iou > np.float32(iou_thres)]
    return np.unique(v).size == v.size
