"""CPU: tests/focal_ref.py (the torch restatement the GPU focal / autobalance tests lean on) reproduces every fixture
that tools/gen_golden.py gen_focal() captured from the reference's own ComputeLoss, at the tolerances of
test_oracle_golden.py::test_oracle_loss, including the autobalance trajectory."""
import pytest
import torch

from focal_ref import FocalComputeLoss
from golden_util import Fixture

SINGLE = ['focal_visdrone', 'focal_scratch_ls', 'focal_g05']
MULTI = ['focal_autobalance', 'focal_autobalance_g0']


def _ref(fx, **kw):
    m = fx.meta
    return FocalComputeLoss(fx.t('anchors'), m['hyp'], m['nc'], m['stride'], **kw)


@pytest.mark.parametrize('name', SINGLE)
def test_helper_reproduces_focal_fixture(name):
    fx = Fixture(name)
    assert fx.meta['hyp']['fl_gamma'] > 0
    pp = [fx.t(f'p.{i}').requires_grad_(True) for i in range(3)]
    loss, items = _ref(fx)(pp, fx.t('targets'))
    loss.backward()
    torch.testing.assert_close(loss, fx.t('loss'), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(items, fx.t('items'), rtol=1e-5, atol=1e-6)
    for i in range(3):
        torch.testing.assert_close(pp[i].grad, fx.t(f'gp.{i}'), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize('name', MULTI)
def test_helper_reproduces_autobalance_trajectory(name):
    fx = Fixture(name)
    ref = _ref(fx, autobalance=True)
    assert ref.ssi == fx.meta['ssi'] == 1
    bal = fx.t('balance')
    assert bal.dtype == torch.float64
    for k in range(fx.meta['calls']):
        pp = [fx.t(f'p.{i}')[k].clone().requires_grad_(True) for i in range(3)]
        loss, items = ref(pp, fx.t('targets'))
        torch.testing.assert_close(loss, fx.t('loss')[k], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(items, fx.t('items')[k], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(torch.tensor(ref.balance, dtype=torch.float64), bal[k], rtol=1e-5, atol=0)
    assert not torch.equal(bal[0], bal[-1])  # the trajectory moves: a frozen balance would not pass
    loss.backward()
    for i in range(3):
        torch.testing.assert_close(pp[i].grad, fx.t(f'gp.{i}'), rtol=1e-4, atol=1e-7)


def test_helper_float64_close_to_float32():
    """the helper runs in float64 with autograd (what the GPU tests use as their reference)"""
    fx = Fixture('focal_g05')
    pp = [fx.t(f'p.{i}').double().requires_grad_(True) for i in range(3)]
    loss, items = _ref(fx)(pp, fx.t('targets'))
    loss.backward()
    assert loss.dtype == torch.float64 and pp[0].grad.dtype == torch.float64
    torch.testing.assert_close(loss.float(), fx.t('loss'), rtol=1e-5, atol=1e-6)
