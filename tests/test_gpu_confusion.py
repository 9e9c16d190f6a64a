"""ConfusionMatrix on the gfx950 kernel (csrc/metrics.hip, dmy_confusion_matrix) against the numpy restatement
tests/confusion_ref.py, which tests/test_confusion_ref.py pins to the reference's own matrices: exact integer equality
on the recorded goldens, hand-built images and a crowded batch, and through val.batch_stats / val.run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confusion_cases as cases  # noqa: E402
import confusion_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = os.path.join(ROOT, 'dma-yolo_amd', 'dmayolo', 'configs', 'yolov5n.yaml')


def _gpu(arrs, width):
    return [torch.tensor(np.asarray(a, np.float32).reshape(-1, width)).cuda() for a in arrs]


def _run(dets, labs, nc, conf, thr, cm=None):
    from dmayolo.utils.metrics import ConfusionMatrix
    cm = cm or ConfusionMatrix(nc, conf=conf, iou_thres=thr)
    cm.process_batch_multi(_gpu(dets, 6), _gpu(labs, 5))
    return cm


def _exact(cm, want):
    got = cm.matrix
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)


@pytest.mark.parametrize('path', cases.GOLDEN, ids=os.path.basename)
def test_kernel_matches_restatement_on_goldens(path):
    dets, labs, nc, conf, thr, want = cases.load_golden(path)
    expect = ref.confusion_matrix(dets, labs, nc, conf, thr)
    assert np.array_equal(expect, want)  # the restatement is the reference's matrix here
    _exact(_run(dets, labs, nc, conf, thr), expect)


@pytest.mark.parametrize('name', sorted(cases.HAND))
def test_hand_cases(name):
    dets, labs, nc, conf, thr, cells = cases.HAND[name]
    d, l = cases.arrays(dets, labs)
    want = cases.dense(nc, cells)
    assert np.array_equal(ref.confusion_matrix([d], [l], nc, conf, thr), want)
    _exact(_run([d], [l], nc, conf, thr), want)


def test_out_of_range_classes_are_not_stored():
    dets, labs, nc, conf, thr, cells = cases.OUT_OF_RANGE
    d, l = cases.arrays(dets, labs)
    _exact(_run([d], [l], nc, conf, thr), cases.dense(nc, cells))


@pytest.fixture(scope='module')
def crowded_batches():
    """nc -> 3 images with uneven offsets; the middle one has 300 detections over 40 labels (more than one pass of
    the 256-thread loops, far more than 16 candidates), the first one two labels without a detection, the last one a
    single label"""
    out = {}
    for nc in (3, 80):
        dets, labs = zip(*[cases.crowded(11 + nc, 17, 5, nc), cases.crowded(12 + nc, 300, 40, nc),
                           cases.crowded(13 + nc, 9, 1, nc)])
        lonely = np.array([[1, 900, 900, 950, 950], [nc - 1, 960, 900, 990, 950]], np.float32)  # no detection near
        out[nc] = (list(dets), [np.concatenate([labs[0], lonely]), labs[1], labs[2]])
    return out


@pytest.mark.parametrize('nc', [3, 80])
def test_crowded_batch_matches_restatement(crowded_batches, nc):
    dets, labs = crowded_batches[nc]
    iou = ref.box_iou(labs[1][:, 1:], dets[1][dets[1][:, 4] > 0.25, :4])
    assert (iou > 0.45).sum() > 16 and dets[1].shape[0] == 300 and labs[1].shape[0] == 40
    want = ref.confusion_matrix(dets, labs, nc)
    assert np.trace(want[:nc, :nc]) > 0 and want[nc].sum() > 0 and want[:, nc].sum() > 0
    _exact(_run(dets, labs, nc, 0.25, 0.45), want)


def test_two_calls_accumulate(crowded_batches):
    dets, labs = crowded_batches[3]
    cm = _run(dets, labs, 3, 0.25, 0.45)
    _run(dets[::-1], labs[::-1], 3, 0.25, 0.45, cm)
    _exact(cm, 2 * ref.confusion_matrix(dets, labs, 3))


def test_single_image_calls_equal_one_batched_call(crowded_batches):
    from dmayolo.utils.metrics import ConfusionMatrix
    dets, labs = crowded_batches[80]
    one = ConfusionMatrix(80)
    for d, l in zip(_gpu(dets, 6), _gpu(labs, 5)):
        assert one.process_batch(d, l) is None
    assert np.array_equal(one.matrix, _run(dets, labs, 80, 0.25, 0.45).matrix)
    _exact(one, ref.confusion_matrix(dets, labs, 80))


def _synthetic_batch():
    """NMS-like outputs for 4 letterboxed images and their pixel-xywh targets: image 1 has labels and no predictions,
    image 2 predictions and no labels; `shapes` carry a real ratio and padding"""
    H, W, nc = 384, 384, 5
    shapes = [((736, 768), ((0.5, 0.5), (0.0, 8.0)))] * 4
    out, targets = [], []
    for si, (nd, nl) in enumerate([(40, 9), (0, 4), (12, 0), (25, 6)]):
        d, l = cases.crowded(50 + si, nd, max(nl, 1), nc)
        out.append(torch.tensor(d[:nd]).cuda())
        if nl:
            xyxy = torch.tensor(l[:, 1:])
            xywh = torch.cat([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1)
            targets.append(torch.cat([torch.full((nl, 1), float(si)), torch.tensor(l[:, :1]), xywh], 1))
    return out, torch.cat(targets).cuda(), (H, W), shapes, nc


def _native_rows(out, targets, hw, shapes):
    """what val.py:254-261 feeds the matching: predictions and labels scaled back to the original image"""
    from dmayolo.utils.general import scale_coords, xywh2xyxy
    dets, labs = [], []
    for si, pred in enumerate(out):
        labels = targets[targets[:, 0] == si, 1:]
        if len(pred) == 0 or len(labels) == 0:
            continue  # val.py:246-249 and :258: neither reaches the confusion matrix
        predn = pred.clone()
        scale_coords(hw, predn[:, :4], shapes[si][0], shapes[si][1])
        tbox = xywh2xyxy(labels[:, 1:5])
        scale_coords(hw, tbox, shapes[si][0], shapes[si][1])
        dets.append(predn.cpu().numpy())
        labs.append(torch.cat((labels[:, 0:1], tbox), 1).cpu().numpy())
    return dets, labs


def test_batch_stats_feeds_the_confusion_matrix(monkeypatch):
    from dmayolo.utils import metrics
    from dmayolo.utils.metrics import ConfusionMatrix
    from dmayolo.val import batch_stats
    out, targets, hw, shapes, nc = _synthetic_batch()
    iouv = torch.linspace(0.5, 0.95, 10).cuda()
    launched = []
    real_call = metrics.call
    monkeypatch.setattr(metrics, 'call', lambda name, *a: (launched.append(name), real_call(name, *a))[1])

    plain = batch_stats([o.clone() for o in out], targets, hw, iouv, shapes)
    assert launched == ['dmy_process_batch']  # without an instance the new kernel is not launched
    cm = ConfusionMatrix(nc)
    with_cm = batch_stats([o.clone() for o in out], targets, hw, iouv, shapes, confusion_matrix=cm)
    assert sorted(launched[1:]) == ['dmy_confusion_matrix', 'dmy_process_batch']

    assert len(plain) == len(with_cm) == 4
    for a, b in zip(plain, with_cm):
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    dets, labs = _native_rows(out, targets, hw, shapes)
    assert len(dets) == 2  # images 0 and 3; the one with labels and no predictions is skipped
    want = ref.confusion_matrix(dets, labs, nc)
    assert want.sum() > 0 and np.trace(want[:nc, :nc]) > 0
    _exact(cm, want)  # image 1's 4 labels, had they been fed, would sit in the background row


def _v5n(seed, nc):
    from dmayolo.models.yolo import Model
    torch.manual_seed(seed)
    m = Model(CFG, nc=nc)
    with torch.no_grad():  # spread a fresh head's scores over (0, 1), as tests/test_gpu_wbf.py does
        for mi in m.model[-1].m:
            mi.weight *= 8
            mi.bias.view(m.model[-1].na, -1)[:, 4] += 4
    return m.cuda()


@pytest.mark.parametrize('path', ['single', 'augment', 'wbf'])
def test_val_run_takes_a_confusion_matrix(path):
    """val.run on its three paths: the statistics do not change, and the matrix is the restatement's over exactly the
    rows the instance was fed (recorded by a subclass before they go to the kernel)"""
    from dmayolo.synthetic import targets as synthetic_targets
    from dmayolo.utils.metrics import ConfusionMatrix
    from dmayolo.val import run

    class Recording(ConfusionMatrix):
        fed = None

        def process_batch_multi(self, detections, labels):
            self.fed = self.fed or ([], [])
            self.fed[0].extend(d.cpu().numpy() for d in detections)
            self.fed[1].extend(l.cpu().numpy() for l in labels)
            return super().process_batch_multi(detections, labels)

    nc, S = 4, 128
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (2, 3, S, S), generator=g, dtype=torch.uint8),
                synthetic_targets(2, nc, per_image=6, seed=3).cpu())]
    model = [_v5n(0, nc), _v5n(1, nc)] if path == 'wbf' else _v5n(0, nc)
    kw = dict(wbf=dict(iou_thr=0.67)) if path == 'wbf' else dict(augment=path == 'augment')
    cm = Recording(nc, conf=0.05, iou_thres=0.1)  # loose thresholds: an untrained model's boxes do match something
    plain = run(model, batches, nc=nc, **kw)
    got = run(model, batches, nc=nc, confusion_matrix=cm, **kw)
    assert plain[0] == got[0] and np.array_equal(plain[1], got[1]) and plain[2] == got[2]
    assert np.array_equal(plain[3], got[3])
    assert cm.fed is not None and all(len(d) and len(l) for d, l in zip(*cm.fed))
    want = ref.confusion_matrix(cm.fed[0], cm.fed[1], nc, 0.05, 0.1)
    assert want[:, :nc].sum() == sum(len(l) for l in cm.fed[1])  # every fed label lands in exactly one cell
    _exact(cm, want)
