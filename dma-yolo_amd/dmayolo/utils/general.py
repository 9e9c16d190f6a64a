"""utils/general.py counterparts on the hot path: make_divisible, box converters, and the
batched gfx950 non_max_suppression (utils/general.py:633-761: label rows, merge-NMS and the criterion NMS included)."""
import math
import os
from itertools import accumulate

import torch

from .._lib import IOU_KIND
from ..functional import call, ptr, stream


def make_divisible(x, divisor):
    """utils/general.py:450-452."""
    return math.ceil(x / divisor) * divisor


def xywh2xyxy(x):
    """utils/general.py:539-546."""
    y = x.clone()
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def xyxy2xywh(x):
    """utils/general.py:529-536."""
    y = x.clone()
    y[:, 0] = (x[:, 0] + x[:, 2]) / 2
    y[:, 1] = (x[:, 1] + x[:, 3]) / 2
    y[:, 2] = x[:, 2] - x[:, 0]
    y[:, 3] = x[:, 3] - x[:, 1]
    return y


def clip_coords(boxes, shape):
    """utils/general.py:620-630 (tensor branch): clamp xyxy boxes to (height, width) in place."""
    boxes[:, 0].clamp_(0, shape[1])
    boxes[:, 1].clamp_(0, shape[0])
    boxes[:, 2].clamp_(0, shape[1])
    boxes[:, 3].clamp_(0, shape[0])


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None):
    """utils/general.py:605-617: xyxy coords from the letterboxed img1_shape back to img0_shape, in place."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    coords[:, [0, 2]] -= pad[0]
    coords[:, [1, 3]] -= pad[1]
    coords[:, :4] /= gain
    clip_coords(coords, img0_shape)
    return coords


def _pow2(n, lo=2048):
    c = lo
    while c < n:
        c <<= 1
    return c


_CAP_HINT = {}  # (A, nc, multi[, 'labels']) -> sort capacity that held every image's candidates last time
_MASK_CAP = []


def _mask_cap():
    """largest sort capacity the bitmask NMS path (dmy_nms_greedy_mask) takes; DMY_NMS_MASK=0 keeps the lazy kernel"""
    if not _MASK_CAP:
        _MASK_CAP.append(call('dmy_nms_mask_rows') if os.environ.get('DMY_NMS_MASK', '1') != '0' else 0)
    return _MASK_CAP[0]


NMS_TYPES = {'iou': IOU_KIND['iou'], 'giou': IOU_KIND['giou'], 'diou': IOU_KIND['diou'], 'ciou': IOU_KIND['ciou']}


def _pack_labels(labels, nimg, dev):
    """the reference's per-image label list (general.py:663-670: one (n_i, 5) tensor [cls, x, y, w, h] in pixels per
    image) -> (lab [sum n_i, 5] fp32 on dev, lab_off [nimg + 1] int32 on dev, max n_i); None without label rows"""
    if labels is None or not len(labels) or not any(len(l) for l in labels):
        return None
    if len(labels) != nimg:
        raise ValueError(f'labels holds {len(labels)} entries for {nimg} images')
    nl = [int(l.shape[0]) for l in labels]
    lab = torch.cat([l[:, :5].detach().float().to(dev) for l in labels if len(l)]).contiguous()
    off = torch.tensor([0, *accumulate(nl)], dtype=torch.int32).to(dev)
    return lab, off, max(nl)


def nms_prepare(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                labels=(), max_det=300, *, merge=False, redundant=True, nms_type='iou'):
    """argument checks and the launch plan of non_max_suppression: (fp32 contiguous prediction, plan dict) -- the
    plan's `cap` is the sort capacity the launch will use (the hint from earlier calls of this shape; with label rows
    the row count includes the longest label list, and the hint has one key of its own per shape, whatever the label
    counts of a batch)"""
    assert 0 <= conf_thres <= 1 and 0 <= iou_thres <= 1
    kind = str(nms_type).lower()
    if kind not in NMS_TYPES:
        raise ValueError(f'nms_type {nms_type!r}: expected one of {sorted(NMS_TYPES)}')
    pred = prediction.detach()
    if pred.dtype != torch.float32:
        pred = pred.float()
    pred = pred.contiguous()
    nimg, A, no = pred.shape
    nc = no - 5
    multi = bool(multi_label and nc > 1)
    cls_ok = None
    if classes is not None:
        cls_ok = torch.zeros(nc, dtype=torch.uint8, device=pred.device)
        cls_ok[torch.tensor([c for c in classes if 0 <= c < nc], dtype=torch.long, device=pred.device)] = 1
    lab = _pack_labels(labels, nimg, pred.device)
    rows = A + (lab[2] if lab else 0)  # label k of an image is row A + k
    key = (A, nc, multi, 'labels') if lab else (A, nc, multi)  # one hint for every label count of the shape
    plan = dict(conf=float(conf_thres), iou=float(iou_thres), multi=multi, cls_ok=cls_ok, agnostic=bool(agnostic),
                max_det=int(max_det), key=key, cap=min(_CAP_HINT.get(key, 2048), _pow2(rows * (nc if multi else 1))),
                lab=lab, kind=NMS_TYPES[kind], merge=bool(merge), redundant=bool(redundant))
    return pred, plan


def nms_buffers(dev, nimg):
    """a private (candidate counter, pinned host counts) pair for a caller that owns them, e.g. a recorded graph
    (infer.GraphedDetector): the counter starts zeroed and every call re-zeroes it, so no other stream can share it"""
    return (torch.zeros(max(nimg, 64), dtype=torch.int32, device=dev),
            torch.zeros(max(2 * nimg, 64), dtype=torch.int32, pin_memory=True))


def nms_launch(pred, plan, cap=None, bufs=None):
    """the NMS kernels of one call at sort capacity `cap`, no host synchronisation (so it can be recorded into a HIP
    graph, infer.GraphedDetector.detect): returns (cnt, out) -- cnt = [candidate counts | keep counts] (int32, in the
    stream's pinned host buffer, or the caller's own `bufs` = nms_buffers(); a device tensor inside a capture that has
    neither), out = (nimg, max_det, 6) rows; nms_finish reads them.  A plan without label rows, merge or a criterion
    other than plain IoU launches the default entries with the arguments they always had; any other plan goes
    through _launch_modes"""
    nimg, A, no = pred.shape
    dev = pred.device
    cap = plan['cap'] if cap is None else cap
    max_nms = 30000
    if bufs is not None:
        ctr, cnt = bufs[0], bufs[1][:2 * nimg]
    else:
        ctr = _nms_counter(dev, nimg)  # zero on entry; the greedy launch hands the counts to cnt and re-zeroes it
        cnt = _nms_host_counts(dev, nimg)  # pinned host memory the scan writes directly: no read-back copy
    if cnt is None:
        cnt = torch.empty(2 * nimg, dtype=torch.int32, device=dev)
    if plan['lab'] is not None or plan['merge'] or plan['kind'] != NMS_TYPES['iou']:
        return cnt, _launch_modes(pred, plan, cap, ctr, cnt, max_nms)
    keys = torch.empty((nimg, cap), dtype=torch.int64, device=dev)
    call('dmy_nms_candidates', ptr(pred), nimg, A, no, plan['conf'], int(plan['multi']), ptr(plan['cls_ok']), ptr(keys),
         cap, ptr(ctr), stream())
    call('dmy_nms_sort', ptr(keys), cap, ptr(ctr), nimg, stream())
    out = torch.empty((nimg, plan['max_det'], 6), dtype=torch.float32, device=dev)
    if cap <= _mask_cap():  # IoU bitmask + one-wave scan (same keep set and order as the lazy greedy kernel)
        mask = torch.empty(nimg * cap * (cap // 64), dtype=torch.int64, device=dev)
        call('dmy_nms_greedy_mask', ptr(pred), nimg, A, no, plan['iou'], int(plan['agnostic']), plan['max_det'],
             max_nms, ptr(keys), cap, ptr(ctr), None, ptr(mask), ptr(out), ptr(cnt[nimg:]), ptr(cnt), stream())
    else:
        boxes = torch.empty((nimg, max_nms, 5), dtype=torch.float32, device=dev)
        call('dmy_nms_greedy', ptr(pred), nimg, A, no, plan['iou'], int(plan['agnostic']), plan['max_det'], max_nms,
             ptr(keys), cap, ptr(ctr), ptr(boxes), ptr(out), ptr(cnt[nimg:]), ptr(cnt), stream())
    return cnt, out


def _launch_modes(pred, plan, cap, ctr, cnt, max_nms):
    """nms_launch's kernels for a call with label rows, a suppression criterion other than plain IoU, or merge-NMS:
    the entries of those modes (dmy_nms_candidates_labels, dmy_nms_greedy_kind / _mask_kind, dmy_nms_merge), as free
    of host synchronisation as the default ones.  With merge the greedy launch leaves its keep counts on the device
    and the candidate counter alone; dmy_nms_merge's last kernel writes the final keep counts and the candidate counts
    to `cnt` and re-zeroes the counter, as the greedy launch does otherwise"""
    nimg, A, no = pred.shape
    dev = pred.device
    lab, off = (plan['lab'][0], plan['lab'][1]) if plan['lab'] is not None else (None, None)
    keys = torch.empty((nimg, cap), dtype=torch.int64, device=dev)
    if lab is not None:
        call('dmy_nms_candidates_labels', ptr(pred), ptr(lab), ptr(off), nimg, A, no, plan['conf'], int(plan['multi']),
             ptr(plan['cls_ok']), ptr(keys), cap, ptr(ctr), stream())
    else:
        call('dmy_nms_candidates', ptr(pred), nimg, A, no, plan['conf'], int(plan['multi']), ptr(plan['cls_ok']),
             ptr(keys), cap, ptr(ctr), stream())
    call('dmy_nms_sort', ptr(keys), cap, ptr(ctr), nimg, stream())
    max_det = plan['max_det']
    out = torch.empty((nimg, max_det, 6), dtype=torch.float32, device=dev)
    merge = plan['merge']
    nk = torch.empty(nimg, dtype=torch.int32, device=dev) if merge else cnt[nimg:]
    head = (plan['kind'], ptr(pred), ptr(lab), ptr(off), nimg, A, no, plan['iou'], int(plan['agnostic']), max_det,
            max_nms, ptr(keys), cap, ptr(ctr))
    tail = (ptr(out), ptr(nk), None if merge else ptr(cnt), stream())
    if cap <= _mask_cap():
        mask = torch.empty(nimg * cap * (cap // 64), dtype=torch.int64, device=dev)
        call('dmy_nms_greedy_mask_kind', *head, ptr(mask), *tail)
    else:
        boxes = torch.empty((nimg, max_nms, 5), dtype=torch.float32, device=dev)
        call('dmy_nms_greedy_kind', *head, ptr(boxes), *tail)
    if merge:
        merged = torch.empty_like(out)
        hits = torch.empty((nimg, max_det), dtype=torch.int32, device=dev)
        call('dmy_nms_merge', ptr(pred), ptr(lab), ptr(off), nimg, A, no, plan['iou'], int(plan['agnostic']), max_det,
             int(plan['redundant']), ptr(keys), cap, ptr(ctr), ptr(nk), ptr(merged), ptr(hits), ptr(out),
             ptr(cnt[nimg:]), ptr(cnt), stream())
    return out


_NMS_CTR = {}
_NMS_HOST = {}


def _nms_host_counts(dev, nimg):
    """[candidate counts | keep counts] of the current stream's calls in pinned host memory (int32, 2 * nimg): the
    greedy / scan kernels store them there, so nms_finish reads them after a stream synchronize instead of a device ->
    host copy.  None during a graph capture that has no buffer yet (the device tensor is used then)"""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    t = _NMS_HOST.get(key)
    if t is None or t.numel() < 2 * nimg:
        if torch.cuda.is_current_stream_capturing():
            return None
        t = _NMS_HOST[key] = torch.zeros(max(2 * nimg, 64), dtype=torch.int32, pin_memory=True)
    return t[:2 * nimg]


def _nms_counter(dev, nimg):
    """the candidate counter of the current stream: int32 [>= nimg], zero between calls (the greedy launch of each call
    copies the counts out and re-zeroes it), so a call needs no fill launch.  One per (device, stream handle) for eager
    calls, which run in issue order on that stream; a recorded graph owns its own pair (nms_buffers).  Created (zeroed) outside graph capture when possible; one created during a capture is
    zeroed by a fill recorded in that graph"""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    t = _NMS_CTR.get(key)
    if t is None or t.numel() < nimg:
        t = torch.zeros(max(nimg, 64), dtype=torch.int32, device=dev)
        if not torch.cuda.is_current_stream_capturing():
            _NMS_CTR[key] = t
    return t


def nms_finish(plan, cap, cnt, out):
    """the one host read of a launch: the per-image detections, or None when some image had more candidates than the
    sort capacity held (the caller reruns at the capacity this records as the new hint)"""
    nimg = out.shape[0]
    if not cnt.is_cuda:  # pinned host counts written by the kernels: wait for them, read them in place
        torch.cuda.current_stream(out.device).synchronize()
    h = cnt.tolist()  # the one host synchronisation
    need = max(h[:nimg])
    if need > cap:
        _CAP_HINT[plan['key']] = _pow2(need)  # overflow: every candidate must enter the sort
        return None
    nk = h[nimg:]
    return [out[b, :nk[b]] for b in range(nimg)]


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                        multi_label=False, labels=(), max_det=300, *, merge=False, redundant=True, nms_type='iou'):
    """Drop-in for utils/general.py:633-761.  Returns a list of (k, 6) tensors [xyxy, conf, cls] on the input
    device, rows in NMS keep order.

    All per-image work runs in three HIP kernels (candidates, bitonic sort, greedy lazy-IoU scan) and the host
    synchronises ONCE per call, reading the candidate counts and keep counts together (one int32 vector).  The
    sort capacity is the power of two that held the previous call's candidates for this prediction shape; when a
    batch overflows it (its true count comes back in the same read) the call reruns once at the exact capacity, so
    the top-`max_nms` cut always sees every candidate (utils/general.py:702-703).

    labels: the autolabel / --save-hybrid input (general.py:663-670, val.py:228-231), one (n_i, 5) tensor
    [cls, x, y, w, h] in pixels per image.  Each row joins the image's candidates after its prediction rows, with
    objectness 1 and a one-hot class, so it scores 1.0 and sorts first (after predictions that score 1.0 too); with
    conf_thres == 1 it is dropped like every other row.  An image with labels and no surviving prediction still has
    output.  A label whose class is outside [0, nc) is dropped (the reference's indexing raises).

    nms_type (case-insensitive) 'iou' | 'giou' | 'diou' | 'ciou': the suppression test between a kept box and a later
    one.  'iou' is torchvision.ops.nms (general.py:708), the call the reference runs.  The others are the reference's
    NMS(boxes, scores, iou_thres, class_nms=...) of general.py:727-761: bbox_iou(kept box, later box) of
    general.py:764-824 with eps on h1, h2 and the union, and the later box stays iff value <= iou_thres (a NaN
    suppresses).  A quirk of the reference that is not copied: NMS() sets SIoU / EIoU flags but never passes them to
    bbox_iou, so its class_nms='SIoU', 'EIoU' and every unknown name run plain IoU; here the four criteria NMS() can
    reach are offered and any other name raises ValueError.

    merge: merge-NMS (general.py:712-718) for images with 1 < n < 3000 candidates: after the cut to max_det every kept
    box becomes the score-weighted mean of all candidates whose plain box_iou with it exceeds iou_thres (fp64 sums,
    rounded to fp32 once); with `redundant`, kept rows that only hit themselves are dropped.  Other images are
    returned unmerged, silently, as in the reference.
    """
    return nms_padded(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, labels, max_det, merge=merge,
                      redundant=redundant, nms_type=nms_type)[1]


def nms_padded(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
               labels=(), max_det=300, *, merge=False, redundant=True, nms_type='iou'):
    """non_max_suppression that also hands back the buffer its result lives in: (out, res) -- out the
    (nimg, max_det, 6) device buffer (None for an empty batch), res the per-image views out[b, :keep count] that
    non_max_suppression returns.  A batched post-process (dmy_scale_boxes) works on `out` with one launch."""
    pred, plan = nms_prepare(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, labels, max_det,
                             merge=merge, redundant=redundant, nms_type=nms_type)
    if pred.shape[0] == 0:
        return None, []
    cap = plan['cap']
    while True:
        cnt, out = nms_launch(pred, plan, cap)
        res = nms_finish(plan, cap, cnt, out)
        if res is not None:
            return out, res
        cap = _CAP_HINT[plan['key']]
