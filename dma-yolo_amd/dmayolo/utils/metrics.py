"""Validation metrics: detection/label matching on the GPU (csrc/metrics.hip)
and the per-class AP integration on the host, as the reference does it.

  process_batch        val.py:62-83 (+ box_iou utils/metrics.py:254-276)  -> dmy_process_batch (HIP)
  process_batch_multi  the same for a whole batch of images in one launch
  ConfusionMatrix      utils/metrics.py:114-189 (its own class-agnostic matching)  -> dmy_confusion_matrix (HIP)
  bbox_iou             utils/metrics.py:192-252 (IoU / GIoU / DIoU / CIoU / SIoU, grad of box1)  -> dmy_bbox_iou_eval (HIP)
  ap_per_class         utils/metrics.py:21-87   (numpy on the host, like the reference: a few thousand
  compute_ap           utils/metrics.py:90-116   scalars per validation run, not a device workload)
  fitness              utils/metrics.py:15-18
"""
import warnings
from pathlib import Path

import numpy as np
import torch

from .._lib import IOU_KIND, call, ptr, stream

_trapz = getattr(np, 'trapezoid', None) or np.trapz  # numpy 2 renamed trapz (same rule)


def _pack(detections, labels, dev):
    """lists of [n_i, 6] detections and [m_i, 5] labels -> (det [ND, 6], lab [NL, 5], det_off, lab_off [B + 1] int32,
    n_i list): the packed batch of the matching kernels, fp32 and contiguous on `dev`"""
    assert len(detections) == len(labels)
    nd = [int(d.shape[0]) for d in detections]
    nl = [int(l.shape[0]) for l in labels]
    det = (torch.cat([d[:, :6].float() for d in detections]) if sum(nd) else torch.zeros(0, 6, device=dev)).contiguous()
    lab = (torch.cat([l[:, :5].float() for l in labels]) if sum(nl) else torch.zeros(0, 5, device=dev)).contiguous()
    offs = torch.tensor(np.concatenate([[0], np.cumsum(nd), [0], np.cumsum(nl)]).astype(np.int32)).to(dev)
    return det, lab, offs[:len(nd) + 1], offs[len(nd) + 1:], nd


def process_batch_multi(detections, labels, iouv):
    """detections: list of [n_i, 6] (x1, y1, x2, y2, conf, cls); labels: list of [m_i, 5] (cls, x1, y1, x2, y2),
    all fp32 on one GPU.  Returns the list of correct [n_i, len(iouv)] bool tensors (val.py:62-83 per image)."""
    assert len(detections) == len(labels)
    dev = iouv.device
    if dev.type != 'cuda':
        raise RuntimeError('process_batch runs on the gfx950 kernel: tensors must be on a GPU')
    T = iouv.numel()
    if sum(int(d.shape[0]) for d in detections) == 0:
        return [torch.zeros(0, T, dtype=torch.bool, device=dev) for _ in detections]
    det, lab, doff, loff, nd = _pack(detections, labels, dev)
    ND = det.shape[0]
    iv = iouv.float().contiguous()
    ws_lab = torch.empty(ND, dtype=torch.int32, device=dev)
    ws_iou = torch.empty(ND, dtype=torch.float32, device=dev)
    ws_win = torch.empty(ND, dtype=torch.int32, device=dev)
    correct = torch.empty((ND, T), dtype=torch.uint8, device=dev)
    call('dmy_process_batch', ptr(det), ptr(doff), ptr(lab), ptr(loff), len(nd), ptr(iv), T, ptr(ws_lab), ptr(ws_iou),
         ptr(ws_win), ptr(correct), stream())
    return list(correct.bool().split(nd))


def process_batch(detections, labels, iouv):
    """val.py:62-83: correct [N, len(iouv)] for one image (detections [N, 6], labels [M, 5], xyxy)."""
    return process_batch_multi([detections], [labels], iouv)[0]


class ConfusionMatrix:
    """utils/metrics.py:114-189 with the matching on the GPU (csrc/metrics.hip states the rules): rows are predicted
    classes, columns true classes, index nc is background.  The counters live on the device of the first batch and
    are only added to there; `.matrix` reads them back, which is the one host synchronisation."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc = nc  # number of classes
        self.conf = conf
        self.iou_thres = iou_thres
        self._counts = None  # [nc + 1, nc + 1] int64 on the GPU, made by the first batch

    @property
    def matrix(self):
        """the (nc + 1, nc + 1) float64 array the reference keeps, read back from the device"""
        if self._counts is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        return self._counts.cpu().numpy().astype(np.float64)

    def process_batch_multi(self, detections, labels):
        """detections: list of [n_i, 6] (x1, y1, x2, y2, conf, cls); labels: list of [m_i, 5] (cls, x1, y1, x2, y2),
        one entry per image, all on one GPU: utils/metrics.py:122-160 for every image in one launch.  Returns None;
        nothing is read back."""
        assert len(detections) == len(labels)
        if not len(detections):
            return
        dev = detections[0].device
        if dev.type != 'cuda':
            raise RuntimeError('ConfusionMatrix runs on the gfx950 kernel: tensors must be on a GPU')
        if self._counts is None:
            self._counts = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int64, device=dev)
        elif self._counts.device != dev:
            raise RuntimeError(f'ConfusionMatrix counts on {self._counts.device}, batch on {dev}')
        det, lab, doff, loff, nd = _pack(detections, labels, dev)
        ND, NL = det.shape[0], lab.shape[0]
        if NL == 0:
            return  # without labels nothing is counted (an image's detections count only once one of them matched)
        ws_lab = torch.empty(max(ND, 1), dtype=torch.int32, device=dev)
        ws_iou = torch.empty(max(ND, 1), dtype=torch.float32, device=dev)
        ws_win = torch.empty(max(ND, 1), dtype=torch.int32, device=dev)
        ws_lab_win = torch.empty(NL, dtype=torch.int32, device=dev)
        call('dmy_confusion_matrix', ptr(det), ptr(doff), ptr(lab), ptr(loff), len(nd), self.nc, self.conf,
             self.iou_thres, ptr(ws_lab), ptr(ws_iou), ptr(ws_win), ptr(ws_lab_win), ptr(self._counts), stream())

    def process_batch(self, detections, labels):
        """utils/metrics.py:122-160 for one image: detections [N, 6], labels [M, 5], xyxy.  Returns None."""
        self.process_batch_multi([detections], [labels])

    def plot(self, normalize=True, save_dir='', names=()):
        """utils/metrics.py:165-185: the heatmap of the (column-normalised) matrix, written to
        save_dir/confusion_matrix.png.  Cells under 0.005 are left blank, cell values are annotated below 30
        classes, the tick labels are `names` + background when there is one name per class (fewer than 99).
        Any failure, a missing plotting library included, is a printed warning and not an error."""
        try:
            import matplotlib.pyplot as plt
            import seaborn as sn

            array = self.matrix
            if normalize:
                array = array / (array.sum(0, keepdims=True) + 1e-6)
            array[array < 0.005] = np.nan
            named = 0 < len(names) < 99 and len(names) == self.nc
            xticks = list(names) + ['background FP'] if named else 'auto'
            yticks = list(names) + ['background FN'] if named else 'auto'
            fig = plt.figure(figsize=(12, 9), tight_layout=True)
            sn.set(font_scale=0.8 if self.nc >= 50 else 1.0)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')  # an all-NaN (empty) matrix warns
                ax = sn.heatmap(array, annot=self.nc < 30, annot_kws={'size': 8}, fmt='.2f', cmap='Blues', square=True,
                                xticklabels=xticks, yticklabels=yticks)
            ax.set_facecolor((1, 1, 1))
            ax.set_xlabel('True')
            ax.set_ylabel('Predicted')
            fig.savefig(Path(save_dir) / 'confusion_matrix.png', dpi=250)
            plt.close()
        except Exception as e:
            print(f'WARNING: ConfusionMatrix plot failure: {e}')

    def print(self):
        """utils/metrics.py:187-189: one line per row, the values separated by blanks"""
        for row in self.matrix:
            print(' '.join(str(v) for v in row))


def iou_kind(GIoU=False, DIoU=False, CIoU=False, SIoU=False):
    """bbox_iou's keywords -> the DMY_IOU_* code, with the precedence of utils/metrics.py:216-252: SIoU first, then
    DIoU before CIoU (metrics.py:241-243), GIoU only when none of those three is set, else the plain IoU"""
    name = 'siou' if SIoU else 'diou' if DIoU else 'ciou' if CIoU else 'giou' if GIoU else 'iou'
    return IOU_KIND[name]


class _BboxIouFn(torch.autograd.Function):
    """value and d iou / d box1 from one dmy_bbox_iou_eval launch (forward-mode duals); backward scales the kept
    gradient by the upstream one"""

    @staticmethod
    def forward(ctx, box1, box2, kind, xyxy):
        n = box2.shape[0]
        ctx.b1_shape = tuple(box1.shape)
        b1 = box1.detach().float()
        b1 = (b1[None].expand(n, 4) if b1.dim() == 1 else b1.t()).contiguous()  # [n, 4] rows, a [4] box broadcast
        b2 = box2.detach().float().contiguous()
        iou = torch.empty(n, dtype=torch.float32, device=b2.device)
        g = torch.empty((n, 4), dtype=torch.float32, device=b2.device)
        call('dmy_bbox_iou_eval', kind, int(bool(xyxy)), ptr(b1), ptr(b2), ptr(iou), ptr(g), n, stream())
        ctx.save_for_backward(g)
        ctx.b1_dtype = box1.dtype
        return iou

    @staticmethod
    def backward(ctx, diou):
        g, = ctx.saved_tensors
        gb = g * diou.float()[:, None]  # [n, 4]
        gb = gb.sum(0) if len(ctx.b1_shape) == 1 else gb.t()
        return gb.to(ctx.b1_dtype), None, None, None


def bbox_iou(box1, box2, x1y1x2y2=True, GIoU=False, DIoU=False, CIoU=False, SIoU=False, eps=1e-7):
    """utils/metrics.py:192-252 on the GPU, through the loss kernel's own device functions (csrc/iou.h):
    box1 is [4] or [4, n], box2 is [n, 4]; the return is [n] fp32.  A [4] box1 is taken against every row of box2.
    x1y1x2y2=True takes the corners as given, False takes (x, y, w, h).  The keywords have the reference's precedence
    (iou_kind above).  Differentiable with respect to box1 (a broadcast [4] box gets the sum over n); the gradient is
    the forward-mode dual of the same evaluation, with the reference's tie rules and CIoU's constant alpha.

    NotImplementedError: box2 requiring grad (box 2 is a constant in the kernel), an eps other than 1e-7 (compiled
    in), CPU tensors (there is no CPU path)."""
    if box1.device.type != 'cuda' or box2.device.type != 'cuda':
        raise NotImplementedError('bbox_iou runs on the gfx950 kernel: tensors must be on a GPU')
    if eps != 1e-7:
        raise NotImplementedError(f'bbox_iou: eps is compiled in as 1e-7, got {eps}')
    if box2.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('bbox_iou: box2 is a constant of the kernel, it cannot require grad')
    if box2.dim() != 2 or box2.shape[1] != 4:
        raise ValueError(f'bbox_iou: box2 must be [n, 4], got {tuple(box2.shape)}')
    n = box2.shape[0]
    if box1.shape[0] != 4 or box1.dim() > 2 or (box1.dim() == 2 and box1.shape[1] != n):
        raise ValueError(f'bbox_iou: box1 must be [4] or [4, {n}], got {tuple(box1.shape)}')
    return _BboxIouFn.apply(box1, box2, iou_kind(GIoU, DIoU, CIoU, SIoU), x1y1x2y2)


def compute_ap(recall, precision):
    """utils/metrics.py:90-116 (101-point COCO interpolation of the precision envelope)."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return _trapz(np.interp(x, mrec, mpre), x), mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls):
    """utils/metrics.py:21-87 without the plots: (p, r, ap [nc, T], f1, unique classes).  p / r / f1 are taken at
    the confidence that maximises the class-mean F1 on the 1000-point grid, as the reference."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = (target_cls == c).sum()
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + 1e-16)
    i = f1.mean(0).argmax()
    return p[:, i], r[:, i], ap, f1[:, i], unique_classes.astype('int32')


def fitness(x):
    """utils/metrics.py:15-18: 0.1 mAP@0.5 + 0.9 mAP@0.5:0.95."""
    w = [0.0, 0.0, 0.1, 0.9]
    return (x[:, :4] * w).sum(1)
