"""utils/loss.py counterpart: anchor-based YOLO loss with SIoU box regression on gfx950.

ComputeLoss(model)(p, targets) -> (loss[1], items[3]) exactly like utils/loss.py:135-218, with
sort_obj_iou forced on (loss.py:191-194) and the in-place gij clamp (loss.py:265-272).  One
autograd Function runs build_targets + per-target SIoU/BCE + dense objectness BCE in HIP kernels
and keeps dL/dp from the forward; backward scales it by the upstream gradient on device.

hyp['fl_gamma'] > 0 wraps both BCE terms in the reference's FocalLoss (utils/loss.py:35-62, 149-152) and
autobalance=True keeps the per-level objectness balance of utils/loss.py:207-212.  Both run in the same
kernels through the dmy_yolo_loss_level_focal / dmy_yolo_loss_finalize_balance entries; the balance is a
float64 device tensor owned by the ComputeLoss object and updated by the finalize kernel, so a step never
reads it back (the reference's .item() per level) and stays graph-capturable.  With fl_gamma == 0 and
autobalance off the original entries run, unchanged.

ComputeLoss(model, iou_type=...) or hyp['iou_type'] picks the box criterion, the keyword of the reference's bbox_iou
call at utils/loss.py:185: 'siou' (the reference's own, the default), 'ciou', 'diou', 'giou' or 'iou'
(utils/metrics.py:192-252).  It is a compile-time parameter of the target kernel, reached through the
dmy_yolo_loss_level_iou / dmy_yolo_loss_level_focal_iou entries; with 'siou' those run the kernels of the original
entries.
"""
import torch

from .._lib import IOU_KIND
from ..functional import call, ptr, stream, dcode
from .torch_utils import de_parallel


def smooth_BCE(eps=0.1):
    """utils/loss.py:13-15."""
    return 1.0 - 0.5 * eps, 0.5 * eps


def _targets_dev(targets, dev):
    return targets.detach().to(device=dev, dtype=torch.float32).contiguous()


def _build_level(targets, nt, anchors_i, na, H, W, anchor_t, dev):
    cap = max(5 * na * nt, 1)
    ii = torch.empty((6, cap), dtype=torch.int32, device=dev)   # b, a, gj, gi, tcls, count(at [5,0])
    tbox = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    anch = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    cnt = ii[5, :1]
    cnt.zero_()
    if nt:
        call('dmy_build_targets', ptr(targets), nt, ptr(anchors_i), na, H, W, float(anchor_t), ptr(ii[0]), ptr(ii[1]),
             ptr(ii[2]), ptr(ii[3]), ptr(ii[4]), ptr(tbox), ptr(anch), ptr(cnt), stream())
    return ii, tbox, anch, cnt, cap


class _YoloLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cl, targets, *p):
        dev = p[0].device
        t = _targets_dev(targets, dev)
        nt = t.shape[0]
        h = cl.hyp
        nl = len(p)
        PR = call('dmy_yolo_loss_part_rows')
        part = torch.zeros(nl * PR, dtype=torch.float32, device=dev)  # per-block partials, fixed-order reduction
        Gs = []
        bs = p[0].shape[0]
        bal = cl._balance_on(dev) if (cl.fl_gamma > 0 or cl.autobalance) else None
        for i, pi in enumerate(p):
            N, na, H, W, no = pi.shape
            assert pi.stride(4) == 1, 'channel dim must be contiguous'
            ii, tbox, anch, cnt, cap = _build_level(t, nt, cl.anchors[i], na, H, W, h['anchor_t'], dev)
            G = torch.zeros_like(pi, dtype=torch.float32)
            tobj = torch.zeros(N * na * H * W, dtype=torch.float32, device=dev)
            tgrad = torch.empty((cap, 4 + (cl.nc if cl.nc > 1 else 0)), dtype=torch.float32, device=dev)
            links = torch.empty(N * na * H * W + cap, dtype=torch.int32, device=dev)
            s = pi.stride()
            head = (dcode(pi), ptr(pi), s[0], s[1], s[2], s[3], N, na, H, W, no, cl.nc, float(h['box']),
                    float(h['obj']), float(h['cls']), float(h['cls_pw']), float(h['obj_pw']), float(cl.cp),
                    float(cl.cn))
            tail = (float(bs), ptr(ii[0]), ptr(ii[1]), ptr(ii[2]), ptr(ii[3]), ptr(ii[4]), ptr(tbox), ptr(anch),
                    ptr(cnt), cap, ptr(G), ptr(tobj), ptr(part[PR * i:]), ptr(tgrad), ptr(links), stream())
            if bal is None:
                call('dmy_yolo_loss_level_iou', *head, float(cl._balance[i]), *tail, cl.iou_kind)
            else:
                call('dmy_yolo_loss_level_focal_iou', *head, ptr(bal), i, float(cl.fl_gamma), *tail, cl.iou_kind)
            Gs.append(G)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        items = torch.empty(3, dtype=torch.float32, device=dev)
        if bal is None:
            call('dmy_yolo_loss_finalize', ptr(part), nl, float(h['box']), float(h['obj']), float(h['cls']),
                 float(bs), ptr(loss), ptr(items), stream())
        else:  # lobj with the balance as it stood before this call, then the autobalance update, all on the device
            call('dmy_yolo_loss_finalize_balance', ptr(part), nl, float(h['box']), float(h['obj']), float(h['cls']),
                 float(bs), ptr(bal), int(cl.autobalance), cl.ssi, ptr(loss), ptr(items), stream())
        ctx.Gs = Gs
        ctx.dtypes = [pi.dtype for pi in p]
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, dloss, ditems):
        dloss = dloss.float().contiguous()
        grads = []
        for G, dt in zip(ctx.Gs, ctx.dtypes):
            dp = torch.empty_like(G, dtype=dt)
            call('dmy_loss_grad', 1 if dt == torch.bfloat16 else 0, ptr(G), ptr(dloss), ptr(dp), G.numel(), stream())
            grads.append(dp)
        ctx.Gs = None
        return (None, None, *grads)


class ComputeLoss:
    """utils/loss.py:135-218 (anchor-based), with the focal wrapper (hyp['fl_gamma'] > 0) and autobalance.

    iou_type (default hyp.get('iou_type', 'siou'), case-insensitive) is the box criterion, named after the keyword
    the reference's `bbox_iou(pbox.T, tbox[i], x1y1x2y2=False, ...)` call at utils/loss.py:185 would carry
    (utils/metrics.py:192-252):
      'siou'  SIoU=True   the reference's own call, the default
      'ciou'  CIoU=True   what upstream YOLOv5 trains with; alpha is a constant, as under the reference's no_grad
      'diou'  DIoU=True
      'giou'  GIoU=True
      'iou'   no keyword  plain intersection over union
    Any other name raises ValueError here, before anything is launched.

    Autobalance deviates from the reference in one place: a level whose objectness loss is exactly 0 (or not
    finite) keeps its balance for that step, where the reference's `0.0001 / obji.item()` raises
    ZeroDivisionError.  Under DDP every rank keeps its own balance, as in the reference."""

    def __init__(self, model, autobalance=False, iou_type=None):
        h = model.hyp
        self.iou_type = str(h.get('iou_type', 'siou') if iou_type is None else iou_type).lower()
        if self.iou_type not in IOU_KIND:
            raise ValueError(f'iou_type {iou_type if iou_type is not None else h.get("iou_type")!r}: '
                             f'expected one of {sorted(IOU_KIND)}')
        self.iou_kind = IOU_KIND[self.iou_type]
        self.fl_gamma = float(h.get('fl_gamma', 0.0))
        assert 0.0 <= self.fl_gamma < float('inf'), f'fl_gamma {self.fl_gamma} must be finite and >= 0'
        self.cp, self.cn = smooth_BCE(eps=h.get('label_smoothing', 0.0))
        det = de_parallel(model).model[-1]
        self._balance = {3: [4.0, 1.0, 0.4]}.get(det.nl, [4.0, 1.0, 0.25, 0.06, 0.02])
        self._balance_dev = None  # float64 on the device once the focal / autobalance path runs
        self.ssi = [float(s) for s in det.stride].index(16.0) if autobalance else 0  # stride 16 index
        self.gr, self.hyp, self.autobalance = 1.0, h, bool(autobalance)
        for k in ('na', 'nc', 'nl'):
            setattr(self, k, getattr(det, k))
        self.anchors = det.anchors.float().contiguous()
        if (self.fl_gamma > 0 or self.autobalance) and self.anchors.is_cuda:
            self._balance_on(self.anchors.device)  # allocated here, so that a first call may already be captured

    def _balance_on(self, dev):
        """the balance as device state: one float64 tensor whose address never changes (graph capture records the
        kernels that read and update it)"""
        if self._balance_dev is None or self._balance_dev.device != dev:
            self._balance_dev = torch.tensor(self.balance, dtype=torch.float64, device=dev)
        return self._balance_dev

    @property
    def balance_dev(self):
        """the float64 device tensor the kernels read and update (None while only the plain path has run);
        reading the attribute does not synchronise"""
        return self._balance_dev

    @property
    def balance(self):
        """per-level objectness balance as a list of floats (utils/loss.py:161).  With autobalance this reads the
        device state back and synchronises; a training step never does."""
        if self.autobalance and self._balance_dev is not None:
            return self._balance_dev.tolist()
        return list(self._balance)

    @balance.setter
    def balance(self, v):
        v = [float(x) for x in v]
        assert len(v) == len(self._balance), (len(v), len(self._balance))  # the device tensor keeps its shape
        self._balance = v
        if self._balance_dev is not None:
            self._balance_dev.copy_(torch.tensor(v, dtype=torch.float64))

    def __call__(self, p, targets):
        return _YoloLossFn.apply(self, targets, *p)

    def build_targets(self, p, targets):
        """utils/loss.py:220-276 on device (the host sync here is for API compatibility only)."""
        dev = p[0].device
        t = _targets_dev(targets, dev)
        tcls, tbox, indices, anch = [], [], [], []
        for i, pi in enumerate(p):
            _, na, H, W, _ = pi.shape
            ii, tb, an, cnt, cap = _build_level(t, t.shape[0], self.anchors[i], na, H, W, self.hyp['anchor_t'], dev)
            n = int(cnt.item())
            iil = ii[:, :n].long()
            indices.append((iil[0], iil[1], iil[2], iil[3]))
            tcls.append(iil[4])
            tbox.append(tb[:n])
            anch.append(an[:n])
        return tcls, tbox, indices, anch
