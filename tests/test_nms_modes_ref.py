"""The CPU restatement of the NMS modes (tests/nms_modes_ref.py) against its own anchors: the oracle for the default
call, and an fp64 evaluation of the merge formula for its fp32 arithmetic."""
import pytest
import torch

import nms_modes_ref as R
from oracle.general import non_max_suppression as onms


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('kw', [dict(), dict(agnostic=True), dict(multi_label=True, classes=[0, 2]),
                                dict(multi_label=True, max_det=7, conf_thres=0.5)])
def test_default_mode_is_the_oracle(seed, kw):
    """nms_type='iou', no labels, no merge: oracle.general.non_max_suppression, row for row"""
    pred = R.cluster_prediction(seed, second=True)
    kw = dict(dict(conf_thres=0.25, iou_thres=0.45), **kw)
    got, ref = R.non_max_suppression(pred, **kw), onms(pred, **kw)
    assert len(got) == len(ref) and sum(len(r) for r in ref) > 0
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_fp32_merge_against_fp64(seed):
    """general.py:716 in the restatement's fp32 arithmetic against the same formula in fp64: per coordinate within
    n * 2^-24 relative, n the number of non-zero weights of the row -- the bound of an fp32 sum of n terms.

    A plain fp32 torch.mm followed by the division does not keep that bound: it rounds up to 2 n times, and on these
    seeds it reached 1.69 and 1.27 times the bound on rows with n = 1 ((w * x) / w rounds twice) and 1.03 on one
    row with n >= 2.  The restatement therefore evaluates the formula with compensated fp32 sums and a corrected
    quotient (nms_modes_ref.merged_boxes): one rounding in all, within the bound for every n >= 1."""
    pred = R.cluster_prediction(seed)
    rows = 0
    for x in R.candidates(pred, 0.25):
        boxes = x[:, :4] + x[:, 5:6] * 4096
        keep = R.greedy_nms_kind(boxes, x[:, 4], 0.45, 'iou', 300)
        hit, w = R.merge_weights(x, keep, 0.45)
        m32, m64 = R.merged_boxes(x, w), R.merged_boxes(x, w, torch.float64)
        n = (w != 0).sum(1, keepdim=True).double()
        err = (m32.double() - m64).abs()
        bound = n * 2.0 ** -24 * m64.abs()
        ratio, one = err / bound, (n == 1).expand_as(err)
        print(seed, 'rows', len(keep), 'n', int(n.min()), int(n.max()), 'worst err / bound', float(ratio.max()),
              'n = 1:', float(ratio[one].max()) if one.any() else None, 'n >= 2:', float(ratio[~one].max()))
        assert bool((err <= bound).all())
        rows += len(keep)
    assert rows > 0
