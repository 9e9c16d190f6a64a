"""Validation loop: the statistics part of the reference's val.run (val.py:196-311) on the gfx950 path.

Per batch: model eval forward (Detect decode) -> non_max_suppression(conf 0.001, iou 0.6, multi_label)
-> labels to pixel xyxy -> process_batch for every image of the batch in ONE kernel launch
(utils/metrics.process_batch_multi) -> (correct, conf, pcls, tcls) stats.  At the end ap_per_class
gives P, R, mAP@0.5 and mAP@0.5:0.95 exactly as val.py:283-291.

Batches are what dmayolo.data.create_dataloader yields (datasets.py:624-629's collate: uint8 images at the
network size [N, 3, H, W], normalised targets [nt, 6] (img, cls, x, y, w, h), paths, shapes), or
(img, targets[, shapes]) tensors; `shapes` (per-image (h0, w0), ((ratio), (pad))) drive scale_coords.

Multi-model ensembles (the reference's val2.py per model -> txt -> wbf.py chain, wbf.py:33-67): run() takes a list of
models plus wbf=dict(iou_thr, skip_box_thr, weights).  Each batch goes through every model and its own NMS, the padded
NMS buffers are fused on the device by weighted boxes fusion over the network-size image (utils/wbf.wbf_padded), and the
statistics are taken from the fused rows.

Confusion matrix (val.py:178, 263-264): run(..., confusion_matrix=utils.metrics.ConfusionMatrix(nc)) feeds the instance
every batch's native-space (predn, labelsn) pairs in one launch, for the images that have both labels and predictions;
the caller reads .matrix / calls .plot() afterwards.  Without an instance nothing of it runs.
save_hybrid (val.py:228-231): run(..., save_hybrid=True) hands the pixel-scaled labels of the batch to
non_max_suppression(labels=...), which appends them to every image's candidates.
Out of scope (control plane): plots, COCO-JSON, txt saving.
"""
import numpy as np
import torch

from .utils.general import nms_padded, non_max_suppression, scale_coords, xywh2xyxy
from .utils.metrics import ap_per_class, process_batch_multi
from .utils.wbf import wbf_padded

WBF_DEFAULTS = dict(iou_thr=0.67, skip_box_thr=0.01, weights=None)  # wbf.py:33-34


def batch_stats(out, targets, img_hw, iouv, shapes=None, single_cls=False, confusion_matrix=None):
    """val.py:236-270 for one batch: NMS outputs `out` (list of [k, 6]), targets [nt, 6] with PIXEL xywh ->
    list of (correct [k, T] bool, conf [k], pcls [k], tcls list) numpy tuples; every image's matching in one
    process_batch launch.  confusion_matrix: a utils.metrics.ConfusionMatrix that takes the same native-space rows
    of every image with labels AND predictions (val.py:258-264: an image with labels and no predictions adds
    nothing to it), in one more launch."""
    device, niou = iouv.device, iouv.numel()
    height, width = img_hw
    stats, dets, labs, tcls_all, keep = [], [], [], [], []
    for si, pred in enumerate(out):
        labels = targets[targets[:, 0] == si, 1:]
        nl = len(labels)
        tcls = labels[:, 0].tolist() if nl else []
        if len(pred) == 0:
            if nl:
                stats.append((np.zeros((0, niou), dtype=bool), np.zeros(0, np.float32), np.zeros(0, np.float32), tcls))
            continue
        if single_cls:
            pred[:, 5] = 0
        predn = pred.clone()
        shape0 = shapes[si][0] if shapes is not None else (height, width)
        ratio_pad = shapes[si][1] if shapes is not None else None
        scale_coords((height, width), predn[:, :4], shape0, ratio_pad)
        if nl:
            tbox = xywh2xyxy(labels[:, 1:5])
            scale_coords((height, width), tbox, shape0, ratio_pad)
            labelsn = torch.cat((labels[:, 0:1], tbox), 1)
        else:
            labelsn = torch.zeros((0, 5), device=device)
        dets.append(predn)
        labs.append(labelsn)
        tcls_all.append(tcls)
        keep.append(pred)
    if confusion_matrix is not None:
        both = [(d, l) for d, l in zip(dets, labs) if len(l)]
        if both:
            confusion_matrix.process_batch_multi(*zip(*both))
    if dets:
        for correct, pred, tcls in zip(process_batch_multi(dets, labs, iouv), keep, tcls_all):
            stats.append((correct.cpu().numpy(), pred[:, 4].float().cpu().numpy(), pred[:, 5].float().cpu().numpy(),
                          tcls))
    return stats


def summarize(stats, nc):
    """val.py:283-291: stats list -> (mp, mr, map50, map, maps [nc], nt [nc])."""
    mp = mr = map50 = map_ = 0.0
    stats = [np.concatenate([np.asarray(s) for s in x], 0) for x in zip(*stats)]
    ap = None
    ap_class = np.zeros(0, dtype=np.int32)
    if len(stats) and stats[0].any():
        p, r, ap, f1, ap_class = ap_per_class(*stats)
        ap50, ap = ap[:, 0], ap.mean(1)
        mp, mr, map50, map_ = p.mean(), r.mean(), ap50.mean(), ap.mean()
        nt = np.bincount(stats[3].astype(np.int64), minlength=nc)
    else:
        nt = np.zeros(nc, dtype=np.int64)
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = ap[i]
    return mp, mr, map50, map_, maps, nt


def fused_detections(outs, img_hw, conf_thres, iou_thres, max_det, single_cls, wbf):
    """the ensemble's post-process for one batch: outs = each model's decoded output -> per model nms_padded, then one
    weighted boxes fusion over the (height, width) network image; returns the per-image fused [k, 6] rows"""
    height, width = img_hw
    bufs, counts = [], []
    for out in outs:
        buf, res = nms_padded(out, conf_thres, iou_thres, multi_label=True, agnostic=single_cls, max_det=max_det)
        bufs.append(buf)
        counts.append([len(r) for r in res])
    nimg = len(counts[0])
    if nimg == 0:
        return []
    dev = bufs[0].device
    wh = torch.tensor([[width, height]] * nimg, dtype=torch.float32, device=dev)
    return wbf_padded(torch.stack(bufs), torch.tensor(counts, dtype=torch.int32, device=dev), wh, wbf['weights'],
                      wbf['iou_thr'], wbf['skip_box_thr'])[1]


@torch.no_grad()
def run(model, batches, nc, conf_thres=0.001, iou_thres=0.6, max_det=300, single_cls=False, compute_loss=None,
        augment=False, wbf=None, confusion_matrix=None, save_hybrid=False):
    """Returns ((mp, mr, map50, map, *loss), maps [nc], seen, nt [nc]) like val.py:303-311.  augment: the model's
    test-time-augmented forward (val.py:213); it has no per-level outputs, so it excludes compute_loss.
    model may be a list or tuple of models with wbf=dict(iou_thr=0.67, skip_box_thr=0.01, weights=None) (missing
    entries take these defaults, wbf.py:33-34): every batch goes through each model and its own NMS, and weighted
    boxes fusion over the network-size image makes the rows the statistics see.  The fused path has no per-level
    outputs either, so it excludes compute_loss.
    confusion_matrix: an optional utils.metrics.ConfusionMatrix, updated in place from every batch (val.py:263-264);
    the return value does not change.
    save_hybrid: the batch's pixel-scaled labels join every image's NMS candidates as apriori rows (val.py:228-231,
    utils.general.non_max_suppression's labels=); the ensemble path has one NMS per model, so it excludes wbf."""
    if save_hybrid and wbf is not None:
        raise ValueError('save_hybrid=True adds the labels to one NMS call: wbf runs one per model (val.py:228-231)')
    if augment and compute_loss:
        raise ValueError('augment=True returns no per-level outputs for compute_loss (val.py:213-217)')
    many = isinstance(model, (list, tuple))
    if many and wbf is None:
        raise ValueError('a list of models needs wbf=dict(...): their detections are fused, not concatenated')
    if wbf is not None and compute_loss:
        raise ValueError('wbf fuses detections of several forwards: there are no per-level outputs for compute_loss')
    if wbf is not None:
        unknown = set(wbf) - set(WBF_DEFAULTS)
        if unknown:
            raise ValueError(f'unknown wbf entries {sorted(unknown)}')
        wbf = {**WBF_DEFAULTS, **wbf}
        models = list(model) if many else [model]
        if not models:
            raise ValueError('an empty list of models')
    else:
        models = [model]
    device = next(models[0].parameters()).device
    was_training = [m.training for m in models]
    for m in models:
        m.eval()
    iouv = torch.linspace(0.5, 0.95, 10, device=device)  # val.py:163
    seen = nbatches = 0
    loss = torch.zeros(3, device=device)
    stats = []
    for batch in batches:
        img, targets = batch[0], batch[1]
        shapes = batch[3] if len(batch) > 3 else (batch[2] if len(batch) > 2 else None)  # (img, t, paths, shapes)
        img = img.to(device, non_blocking=True)
        targets = targets.to(device).float()
        nb, _, height, width = img.shape
        if wbf is not None:
            outs = [(m(img, augment=True) if augment else m(img))[0] for m in models]
        else:
            out, train_out = model(img, augment=True) if augment else model(img)
        if compute_loss:
            loss += compute_loss([x.float() for x in train_out], targets)[1]
        targets[:, 2:] *= torch.tensor([width, height, width, height], device=device, dtype=torch.float32)
        if wbf is not None:
            out = fused_detections(outs, (height, width), conf_thres, iou_thres, max_det, single_cls, wbf)
        else:
            apriori = [targets[targets[:, 0] == si, 1:] for si in range(nb)] if save_hybrid else ()  # pixel (cls, xywh)
            out = non_max_suppression(out, conf_thres, iou_thres, labels=apriori, multi_label=True, agnostic=single_cls,
                                      max_det=max_det)
        nbatches += 1
        seen += len(out)
        stats += batch_stats(out, targets, (height, width), iouv, shapes, single_cls, confusion_matrix)
    mp, mr, map50, map_, maps, nt = summarize(stats, nc)
    for m, t in zip(models, was_training):
        m.train(t)
    loss_items = (loss.cpu() / max(nbatches, 1)).tolist()
    return (mp, mr, map50, map_, *loss_items), maps, seen, nt
