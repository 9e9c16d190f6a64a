"""GPU: the IoU-family box criteria (CIoU / DIoU / GIoU / plain IoU next to SIoU) on the HIP path.

Kernel level (dmy_bbox_iou_eval, the loss kernel's own device functions) and the public
dmayolo.utils.metrics.bbox_iou against the reference's bbox_iou fixtures of tools/gen_golden_iou.py, at siou.npz's
tolerances (value rtol 1e-5 atol 1e-6, gradient rtol 1e-3 atol 1e-4, every row); ComputeLoss(iou_type=...) against
the reference's ComputeLoss fixtures at test_gpu_loss_nms.py::test_loss_and_grad's (loss / items rtol 1e-5 atol 1e-6,
dL/dp rtol 1e-4 atol 1e-6 * max(1, |g|max)); and the contracts around them: SIoU keeps its bits, the default is
unchanged, run-to-run bit equality, graph capture."""
import types

import pytest
import torch

from golden_util import Fixture
from iou_ref import KINDS, bbox_iou_ref

pytestmark = pytest.mark.gpu
CODE = {'siou': 0, 'ciou': 1, 'diou': 2, 'giou': 3, 'iou': 4}
FLAG = {'siou': dict(SIoU=True), 'ciou': dict(CIoU=True), 'diou': dict(DIoU=True), 'giou': dict(GIoU=True), 'iou': {}}
FORMS = [('', False), ('x', True)]
LOSS_CASES = ['ciou', 'giou', 'diou', 'iou', 'ciou_focal', 'ciou_nc1']


def _eval(kind, xyxy, b1, b2):
    from dmayolo.functional import call, ptr, stream
    b1, b2 = b1.cuda().contiguous(), b2.cuda().contiguous()
    n = b1.shape[0]
    iou = torch.empty(n, device='cuda')
    g = torch.empty(n, 4, device='cuda')
    call('dmy_bbox_iou_eval', CODE[kind], int(xyxy), ptr(b1), ptr(b2), ptr(iou), ptr(g), n, stream())
    return iou.cpu(), g.cpu()


def _close(iou, g, ref_iou, ref_g):
    assert bool(torch.isfinite(iou).all()) and bool(torch.isfinite(g).all())
    torch.testing.assert_close(iou, ref_iou, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(g, ref_g, rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------- 1. kernel level
@pytest.mark.parametrize('sfx,xyxy', FORMS)
@pytest.mark.parametrize('kind', KINDS)
def test_bbox_iou_eval_vs_reference(kind, sfx, xyxy):
    fx = Fixture(f'bbox_iou_{kind}')
    iou, g = _eval(kind, xyxy, fx.t(f'b1{sfx}'), fx.t(f'b2{sfx}'))
    print(kind, xyxy, 'max |d iou|', float((iou - fx.t(f'iou{sfx}')).abs().max()), 'max |d g|',
          float((g - fx.t(f'g{sfx}')).abs().max()))
    _close(iou, g, fx.t(f'iou{sfx}'), fx.t(f'g{sfx}'))


def test_kind0_is_siou_eval_bit_for_bit():
    from dmayolo.functional import call, ptr, stream
    fx = Fixture('siou')
    b1, b2 = fx.t('b1').cuda().contiguous(), fx.t('b2').cuda().contiguous()
    n = b1.shape[0]
    iou = torch.empty(n, device='cuda')
    g = torch.empty(n, 4, device='cuda')
    call('dmy_siou_eval', ptr(b1), ptr(b2), ptr(iou), ptr(g), n, stream())
    iou2, g2 = _eval('siou', False, fx.t('b1'), fx.t('b2'))
    ok = torch.isfinite(iou.cpu()) & torch.isfinite(g.cpu()).all(1) & torch.isfinite(fx.t('g')).all(1)
    assert int(ok.sum()) > 200
    assert torch.equal(iou.cpu()[ok], iou2[ok]) and torch.equal(g.cpu()[ok], g2[ok])


# ---------------------------------------------------------------- 2. public function
@pytest.mark.parametrize('sfx,xyxy', FORMS)
@pytest.mark.parametrize('kind', KINDS)
def test_public_bbox_iou_value_and_grad(kind, sfx, xyxy):
    from dmayolo.utils.metrics import bbox_iou
    fx = Fixture(f'bbox_iou_{kind}')
    b1 = fx.t(f'b1{sfx}').cuda().requires_grad_(True)
    iou = bbox_iou(b1.T, fx.t(f'b2{sfx}').cuda(), x1y1x2y2=xyxy, **FLAG[kind])
    assert iou.shape == (256,) and iou.dtype == torch.float32
    iou.sum().backward()
    _close(iou.detach().cpu(), b1.grad.cpu(), fx.t(f'iou{sfx}'), fx.t(f'g{sfx}'))


@pytest.mark.parametrize('sfx,xyxy', FORMS)
@pytest.mark.parametrize('kind', KINDS)
def test_public_bbox_iou_broadcast_box1(kind, sfx, xyxy):
    """one [4] box against the fixture's first 16 box-2 rows (the edge rows); its gradient is the sum over the rows.
    Reference: tests/iou_ref.py in float64 (pinned to the fixtures by test_iou_ref.py)"""
    from dmayolo.utils.metrics import bbox_iou
    fx = Fixture(f'bbox_iou_{kind}')
    b2 = fx.t(f'b2{sfx}')[:16]
    one = fx.t(f'b1{sfx}')[7]
    a = one.double()[None].repeat(16, 1).requires_grad_(True)
    ref = bbox_iou_ref(a, b2.double(), kind, xyxy=xyxy)
    ref.sum().backward()
    b1 = one.cuda().requires_grad_(True)
    iou = bbox_iou(b1, b2.cuda(), x1y1x2y2=xyxy, **FLAG[kind])
    assert iou.shape == (16,)
    iou.sum().backward()
    assert b1.grad.shape == (4,)
    _close(iou.detach().cpu(), b1.grad.cpu(), ref.detach().float(), a.grad.sum(0).float())


def test_public_bbox_iou_flags_and_refusals():
    from dmayolo.utils.metrics import bbox_iou
    fx = Fixture('siou')
    b1, b2 = fx.t('b1').cuda(), fx.t('b2').cuda()
    ok = torch.isfinite(fx.t('g')).all(1)
    s = bbox_iou(b1.T, b2, x1y1x2y2=False, SIoU=True, CIoU=True, GIoU=True).cpu()   # SIoU first
    s0, _ = _eval('siou', False, fx.t('b1'), fx.t('b2'))
    assert torch.equal(s[ok], s0[ok])
    d = bbox_iou(b1.T, b2, x1y1x2y2=False, DIoU=True, CIoU=True, GIoU=True)          # DIoU before CIoU, GIoU last
    assert torch.equal(d, bbox_iou(b1.T, b2, x1y1x2y2=False, DIoU=True))
    assert not torch.equal(d, bbox_iou(b1.T, b2, x1y1x2y2=False, CIoU=True))
    # an upstream gradient other than ones scales the rows
    a = b1.clone().requires_grad_(True)
    up = torch.linspace(-1, 2, 256, device='cuda')
    (bbox_iou(a.T, b2, x1y1x2y2=False, CIoU=True) * up).sum().backward()
    _, g = _eval('ciou', False, fx.t('b1'), fx.t('b2'))
    assert torch.equal(a.grad.cpu(), g * up.cpu()[:, None])
    with pytest.raises(NotImplementedError):
        bbox_iou(b1.T, b2.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        bbox_iou(b1.T, b2, eps=1e-9)
    with pytest.raises(NotImplementedError):
        bbox_iou(b1.T.cpu(), b2)


# ---------------------------------------------------------------- 3. the loss
def _loss_obj(fx, **kw):
    from dmayolo.utils.loss import ComputeLoss
    meta = fx.meta
    det = types.SimpleNamespace(nl=3, na=3, nc=meta['nc'], anchors=fx.t('anchors').cuda(),
                                stride=torch.tensor(meta['stride'], dtype=torch.float32))
    hyp = dict(meta['hyp'], **kw.pop('hyp', {}))
    return ComputeLoss(types.SimpleNamespace(hyp=hyp, model=[det]), **kw)


def _run(cl, ps, targets):
    ps = [p.detach().requires_grad_(True) for p in ps]
    loss, items = cl(ps, targets)
    loss.backward()
    return loss.detach(), items, [p.grad for p in ps]


@pytest.mark.parametrize('layout', ['contiguous', 'nhwc'])
@pytest.mark.parametrize('case', LOSS_CASES)
def test_loss_and_grad_vs_reference(case, layout):
    fx = Fixture(f'loss_{case}')
    cl = _loss_obj(fx, iou_type=fx.meta['iou_type'])
    assert (cl.fl_gamma > 0) == (case == 'ciou_focal') and (cl.nc == 1) == (case == 'ciou_nc1')
    ps = []
    for i in range(3):
        p = fx.t(f'p.{i}').cuda()
        if layout == 'nhwc':  # the Detect head's native layout: [N,H,W,na,no] permuted view
            p = p.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
        ps.append(p)
    loss, items, grads = _run(cl, ps, fx.t('targets').cuda())
    print(case, layout, 'loss', float(loss), float(fx.t('loss')), 'items', items.tolist(), fx.t('items').tolist())
    torch.testing.assert_close(loss.cpu(), fx.t('loss'), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(items.cpu(), fx.t('items'), rtol=1e-5, atol=1e-6)
    if case == 'ciou_nc1':
        assert float(items[2]) == 0.0
    for i in range(3):
        g = fx.t(f'gp.{i}')
        assert bool(torch.isfinite(grads[i]).all())
        torch.testing.assert_close(grads[i].cpu(), g, rtol=1e-4, atol=1e-6 * max(1.0, float(g.abs().max())))


@pytest.mark.parametrize('kind', KINDS)
def test_loss_no_targets(kind):
    fx = Fixture('loss_ciou')
    ps = [fx.t(f'p.{i}').cuda() for i in range(3)]
    loss, items, grads = _run(_loss_obj(fx, iou_type=kind), ps, torch.zeros((0, 6), device='cuda'))
    assert float(items[0]) == 0.0 and float(items[2]) == 0.0
    assert bool(torch.isfinite(loss).all()) and float(loss) > 0 and all(bool(torch.isfinite(g).all()) for g in grads)


# ---------------------------------------------------------------- 4. default unchanged, determinism, capture
def test_default_is_siou_bit_for_bit():
    fx = Fixture('loss_VisDrone')
    ps = [fx.t(f'p.{i}').cuda() for i in range(3)]
    t = fx.t('targets').cuda()
    base = _run(_loss_obj(fx), ps, t)
    assert _loss_obj(fx).iou_type == 'siou'
    for cl in (_loss_obj(fx, iou_type='siou'), _loss_obj(fx, iou_type='SIoU'), _loss_obj(fx, hyp=dict(iou_type='siou'))):
        loss, items, grads = _run(cl, ps, t)
        assert torch.equal(loss, base[0]) and torch.equal(items, base[1])
        assert all(torch.equal(a, b) for a, b in zip(grads, base[2]))
    # the hyp key selects the criterion like the argument does, and another criterion is another loss
    a = _run(_loss_obj(fx, hyp=dict(iou_type='ciou')), ps, t)
    b = _run(_loss_obj(fx, iou_type='ciou'), ps, t)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert not torch.equal(a[0], base[0])


def test_ciou_bitwise_repeatable():
    fx = Fixture('loss_ciou')
    ps = [fx.t(f'p.{i}').cuda() for i in range(3)]
    t = fx.t('targets').cuda()
    a = _run(_loss_obj(fx, iou_type='ciou'), ps, t)
    b = _run(_loss_obj(fx, iou_type='ciou'), ps, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_trainer_hyp_key_reaches_the_loss():
    import os
    from dmayolo.models.yolo import Model
    from dmayolo.synthetic import HYP_VISDRONE, scaled_hyp
    from dmayolo.trainer import Trainer
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dma-yolo_amd', 'dmayolo', 'configs')
    m = Model(os.path.join(cfg, 'yolov5n.yaml'), nc=10, act_dtype=torch.float32).cuda().train()
    m.hyp = dict(scaled_hyp(HYP_VISDRONE, 10, 64, 3), iou_type='CIoU')
    tr = Trainer(m, m.hyp, batch_size=2, epochs=2, nb=2, ema=False, amp=False)
    assert tr.compute_loss.iou_type == 'ciou' and tr.compute_loss.iou_kind == CODE['ciou']


def test_ciou_focal_graph_capture_matches_eager():
    """the loss and its backward recorded into one graph (capture raises on any host synchronisation); a replay gives
    the eager bits"""
    fx = Fixture('loss_ciou_focal')
    t = fx.t('targets').cuda()
    eager = _run(_loss_obj(fx, iou_type='ciou'), [fx.t(f'p.{i}').cuda() for i in range(3)], t)
    cl = _loss_obj(fx, iou_type='ciou')
    sp = [fx.t(f'p.{i}').cuda().requires_grad_(True) for i in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, items = cl(sp, t)
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), eager[0]) and torch.equal(items, eager[1])
    assert all(torch.equal(p.grad, g) for p, g in zip(sp, eager[2]))
