"""CPU: tests/iou_ref.py (the float64 restatement of GIoU / DIoU / CIoU / plain IoU) reproduces the fixtures that
tools/gen_golden_iou.py captured from the reference's own bbox_iou, value and autograd gradient, in both input forms;
and with it in place of SIoU, tests/focal_ref.py reproduces the loss_<kind> fixtures of the reference's ComputeLoss.
That pins the fixtures independently of the kernels.  Tolerances: siou.npz's (value rtol 1e-5 atol 1e-6, gradient
rtol 1e-3 atol 1e-4) and test_focal_ref.py's."""
import pytest
import torch

import focal_ref
from golden_util import Fixture
from iou_ref import KINDS, bbox_iou_ref

LOSS_CASES = ['ciou', 'giou', 'diou', 'iou', 'ciou_focal', 'ciou_nc1']
FORMS = [('', False), ('x', True)]


@pytest.mark.parametrize('kind', KINDS)
def test_fixtures_are_finite_and_hold_the_edge_rows(kind):
    fx = Fixture(f'bbox_iou_{kind}')
    for k in fx.z.files:
        assert bool(torch.isfinite(fx.t(k)).all()), k
    b1, b2 = fx.t('b1'), fx.t('b2')
    assert b1.shape == b2.shape == (256, 4) and fx.t('g').shape == (256, 4) and fx.t('iou').shape == (256,)
    assert bool((b1[:, 2:] > 0).all()) and bool((b2[:, 2:] > 0).all())
    x1, x2 = fx.t('b1x'), fx.t('b2x')
    iou = fx.t('iou')
    assert float(iou[0]) <= 0 and float(iou[1]) <= 0                  # disjoint
    assert float(x1[2, 2]) == float(x2[2, 0]) and bool((x1[2, [1, 3]] == x2[2, [1, 3]]).all())  # touching along an edge
    assert torch.equal(b1[4], b2[4]) and torch.equal(b1[5], b2[5]) and float(iou[4]) > 0.999  # identical
    assert bool((x1[6, :2] > x2[6, :2]).all()) and bool((x1[6, 2:] < x2[6, 2:]).all())       # nested
    assert float(b1[10, 2]) == float(b2[10, 2]) and float(b1[10, 3]) != float(b2[10, 3])     # equal widths
    assert abs(float(b1[12, 2]) - 0.05) < 1e-6 and float(b2[12, 2]) == 3.0                    # sliver against 3-wide


@pytest.mark.parametrize('name', [f'loss_{c}' for c in LOSS_CASES])
def test_loss_fixtures_are_finite(name):
    fx = Fixture(name)
    for k in fx.z.files:
        if k != 'meta':
            assert bool(torch.isfinite(fx.t(k)).all()), k


@pytest.mark.parametrize('sfx,xyxy', FORMS)
@pytest.mark.parametrize('kind', KINDS)
def test_ref_reproduces_bbox_iou_fixture(kind, sfx, xyxy):
    fx = Fixture(f'bbox_iou_{kind}')
    a = fx.t(f'b1{sfx}').double().requires_grad_(True)
    iou = bbox_iou_ref(a, fx.t(f'b2{sfx}').double(), kind, xyxy=xyxy)
    iou.sum().backward()
    iou = iou.detach()
    assert iou.dtype == torch.float64
    print(kind, xyxy, 'max |d iou|', float((iou.float() - fx.t(f'iou{sfx}')).abs().max()), 'max |d g|',
          float((a.grad.float() - fx.t(f'g{sfx}')).abs().max()))
    torch.testing.assert_close(iou.float(), fx.t(f'iou{sfx}'), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(a.grad.float(), fx.t(f'g{sfx}'), rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize('case', LOSS_CASES)
def test_ref_reproduces_loss_fixture(case, monkeypatch):
    fx = Fixture(f'loss_{case}')
    m = fx.meta
    kind = m['iou_type']
    assert kind == case.split('_')[0]
    assert (m['hyp']['fl_gamma'] > 0) == (case == 'ciou_focal') and (m['nc'] == 1) == (case == 'ciou_nc1')
    monkeypatch.setattr(focal_ref, 'siou', lambda b1, b2: bbox_iou_ref(b1, b2, kind))
    ref = focal_ref.FocalComputeLoss(fx.t('anchors'), m['hyp'], m['nc'], m['stride'])
    pp = [fx.t(f'p.{i}').requires_grad_(True) for i in range(3)]
    loss, items = ref(pp, fx.t('targets'))
    loss.backward()
    torch.testing.assert_close(loss, fx.t('loss'), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(items, fx.t('items'), rtol=1e-5, atol=1e-6)
    for i in range(3):
        torch.testing.assert_close(pp[i].grad, fx.t(f'gp.{i}'), rtol=1e-4, atol=1e-7)
