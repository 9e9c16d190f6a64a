"""Weighted boxes fusion on the gfx950 path: ensemble_boxes.weighted_boxes_fusion (conf_type 'avg',
allows_overflow False) as the reference's multi-model evaluation uses it (wbf.py:67), csrc/wbf.hip.

wbf_padded fuses the padded NMS outputs of M models for a whole batch in four launches and one host read;
weighted_boxes_fusion is the library's one-image signature on top of it.  The arithmetic is fp64 on the fp32 rows the
NMS kernels produce, bit for bit the host restatement's (tests/wbf_ref.py).
"""
import numpy as np
import torch

from ..functional import call, ptr, stream

_MAX_ROWS = []


def max_rows():
    """the most records (models x rows) per image the kernels take"""
    if not _MAX_ROWS:
        _MAX_ROWS.append(call('dmy_wbf_max_rows'))
    return _MAX_ROWS[0]


def _check_capacity(M, nimg, R):
    if M * R > max_rows():
        raise NotImplementedError(f'weighted boxes fusion takes at most {max_rows()} rows per image '
                                  f'(models x rows), got {M} x {R}')
    if nimg > 65535:
        raise NotImplementedError(f'weighted boxes fusion takes at most 65535 images per call, got {nimg}')


def wbf_padded(dets, counts, wh, weights=None, iou_thr=0.55, skip_box_thr=0.0):
    """dets (M, nimg, R, 6) fp32 [xyxy px, conf, cls] (nms_padded's buffers stacked over M models), counts (M, nimg)
    int32 valid rows, wh (nimg, 2) image (width, height), weights [M] (default ones) -> (out, res) like nms_padded:
    out the (nimg, M * R, 6) device buffer of fused rows [xyxy px, score, label] in descending score order, res the
    per-image views out[b, :count].  One host synchronisation, the read of the counts."""
    assert 0 <= iou_thr <= 1
    M, nimg, R, six = dets.shape
    assert six == 6 and tuple(counts.shape) == (M, nimg) and tuple(wh.shape) == (nimg, 2)
    _check_capacity(M, nimg, R)  # before any launch: nothing is ever truncated
    if weights is None:
        weights = [1.0] * M
    if len(weights) != M:
        raise ValueError(f'{len(weights)} weights for {M} models')
    dev = dets.device
    if nimg == 0 or M * R == 0:
        return None, [dets.new_zeros((0, 6)) for _ in range(nimg)]
    dets = dets.detach().to(torch.float32).contiguous()
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    wh = torch.as_tensor(wh).to(device=dev, dtype=torch.float32).contiguous()
    w = torch.tensor([float(v) for v in weights], dtype=torch.float64).to(dev)
    ws = torch.empty(call('dmy_wbf_workspace_bytes', nimg, M * R), dtype=torch.uint8, device=dev)
    out = torch.empty((nimg, M * R, 6), dtype=torch.float32, device=dev)
    nout = torch.empty(nimg, dtype=torch.int32, device=dev)
    call('dmy_wbf', ptr(dets), ptr(counts), ptr(wh), ptr(w), M, nimg, R, float(iou_thr), float(skip_box_thr), ptr(ws),
         ptr(out), ptr(nout), stream())
    n = nout.tolist()  # the one host synchronisation
    return out, [out[b, :n[b]] for b in range(nimg)]


def weighted_boxes_fusion(boxes_list, scores_list, labels_list, weights=None, iou_thr=0.55, skip_box_thr=0.0,
                          conf_type='avg', allows_overflow=False, device='cuda'):
    """ensemble_boxes.weighted_boxes_fusion for one image: per model a list / array / tensor of normalised xyxy boxes,
    of scores and of labels -> (boxes [k, 4], scores [k], labels [k]) numpy float32 arrays in descending score order.
    The inputs are rounded to fp32 (the detectors' own precision) before the fp64 fusion."""
    if conf_type != 'avg':
        raise NotImplementedError(f"conf_type '{conf_type}': only 'avg' is built (wbf.py:67 uses the default)")
    if allows_overflow:
        raise NotImplementedError('allows_overflow=True is not built (wbf.py:67 uses the default)')
    M = len(boxes_list)
    if len(scores_list) != M or len(labels_list) != M:
        raise ValueError('boxes_list, scores_list and labels_list differ in length')
    if weights is not None and len(weights) != M:
        raise ValueError(f'{len(weights)} weights for {M} models')

    def arr(x, cols):
        x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        return x.astype(np.float32).reshape((-1, cols) if cols else (-1,))
    rows = []
    for b, s, l in zip(boxes_list, scores_list, labels_list):
        b, s, l = arr(b, 4), arr(s, 0), arr(l, 0)
        if not len(b) == len(s) == len(l):
            raise ValueError('a model has different numbers of boxes, scores and labels')
        rows.append(np.concatenate((b, s[:, None], l[:, None]), 1))
    R = max((len(r) for r in rows), default=0)
    _check_capacity(M, 1, R)
    empty = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    if M == 0 or R == 0:
        return empty
    dets = np.zeros((M, 1, R, 6), np.float32)
    for t, r in enumerate(rows):
        dets[t, 0, :len(r)] = r
    counts = torch.tensor([[len(r)] for r in rows], dtype=torch.int32)
    res = wbf_padded(torch.from_numpy(dets).to(device), counts.to(device), torch.ones((1, 2), device=device), weights,
                     iou_thr, skip_box_thr)[1][0].cpu().numpy()
    return res[:, :4].copy(), res[:, 4].copy(), res[:, 5].copy()
