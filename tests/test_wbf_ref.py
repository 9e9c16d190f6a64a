"""CPU: known answers that pin the weighted-boxes-fusion restatement (tests/wbf_ref.py) itself, so the device kernel
(tests/test_gpu_wbf.py) is not only compared with code written by the same hand; plus what the Python surface refuses
before it touches a device.  All cases are normalised boxes with iou_thr 0.55 unless the case says otherwise."""
import numpy as np
import pytest
import torch

from wbf_ref import weighted_boxes_fusion_ref

# name -> (boxes_list, scores_list, labels_list, iou_thr); shared with the device test of the library-signature wrapper
CASES = {
    'same_box_two_models': ([[[0.1, 0.1, 0.5, 0.5]], [[0.1, 0.1, 0.5, 0.5]]], [[0.8], [0.6]], [[0], [0]], 0.55),
    'one_model_silent': ([[[0.2, 0.2, 0.6, 0.7]], []], [[0.9], []], [[1], []], 0.55),
    'fuse_within_model': ([[[0, 0, 0.4, 0.4], [0, 0, 0.5, 0.4]]], [[0.9, 0.3]], [[0, 0]], 0.55),
    'labels_apart': ([[[0, 0, 0.4, 0.4], [0, 0, 0.5, 0.4]]], [[0.9, 0.3]], [[0, 1]], 0.55),
    'iou_equals_threshold': ([[[0, 0, 0.5, 0.5], [0, 0, 0.5, 0.25]]], [[0.9, 0.3]], [[0, 0]], 0.5),
    'degenerate_and_swapped': ([[[-0.2, 0.3, 0.3, 0.3], [0.6, 0.1, 0.2, 0.5]]], [[0.9, 0.5]], [[0, 0]], 0.55),
}


def _run(name):
    b, s, l, thr = CASES[name]
    return weighted_boxes_fusion_ref(b, s, l, iou_thr=thr)


def test_same_box_two_models():
    boxes, scores, labels = _run('same_box_two_models')
    assert boxes.shape == (1, 4)
    assert np.array_equal(boxes[0], np.float32([0.1, 0.1, 0.5, 0.5]))  # unchanged
    assert scores[0] == pytest.approx(0.7, abs=1e-6) and labels[0] == 0


def test_box_in_one_of_two_models():
    boxes, scores, labels = _run('one_model_silent')
    assert boxes.shape == (1, 4) and np.array_equal(boxes[0], np.float32([0.2, 0.2, 0.6, 0.7]))
    assert scores[0] == pytest.approx(0.45, abs=1e-6) and labels[0] == 1


def test_two_boxes_of_one_model_fuse():
    boxes, scores, labels = _run('fuse_within_model')  # IoU 0.8
    assert boxes.shape == (1, 4)
    assert boxes[0] == pytest.approx([0, 0, 0.425, 0.4], abs=1e-6)  # x2 = (0.9 * 0.4 + 0.3 * 0.5) / 1.2
    assert scores[0] == pytest.approx(0.6, abs=1e-6)  # 1.2 / 2 * min(2, 1) / 1


def test_labels_never_interact():
    boxes, scores, labels = _run('labels_apart')
    assert boxes.shape == (2, 4)
    assert list(labels) == [0, 1] and scores == pytest.approx([0.9, 0.3], abs=1e-6)
    assert np.array_equal(boxes, np.float32([[0, 0, 0.4, 0.4], [0, 0, 0.5, 0.4]]))


def test_comparison_with_threshold_is_strict():
    boxes, scores, labels = _run('iou_equals_threshold')  # IoU exactly 0.5 (0.125 / 0.25) at iou_thr 0.5
    assert boxes.shape == (2, 4) and scores == pytest.approx([0.9, 0.3], abs=1e-6)
    b, s, l, _ = CASES['iou_equals_threshold']
    assert weighted_boxes_fusion_ref(b, s, l, iou_thr=0.49)[0].shape == (1, 4)  # below it they do fuse


def test_degenerate_dropped_swapped_kept():
    boxes, scores, labels = _run('degenerate_and_swapped')
    assert boxes.shape == (1, 4)  # [-0.2, 0.3, 0.3, 0.3] has no area after the clamp
    assert np.array_equal(boxes[0], np.float32([0.2, 0.1, 0.6, 0.5]))  # x2 < x1: swapped, not dropped
    assert scores[0] == pytest.approx(0.5, abs=1e-6)


# ---------------------------------------------------------------- refusals that need no GPU
def test_weighted_boxes_fusion_refuses_other_variants():
    from dmayolo.utils.wbf import weighted_boxes_fusion
    b, s, l, _ = CASES['same_box_two_models']
    for conf_type in ('max', 'box_and_model_avg', 'absent_model_aware_avg'):
        with pytest.raises(NotImplementedError):
            weighted_boxes_fusion(b, s, l, conf_type=conf_type)
    with pytest.raises(NotImplementedError):
        weighted_boxes_fusion(b, s, l, allows_overflow=True)


def test_val_run_refuses_list_without_wbf_and_wbf_with_loss():
    from dmayolo.val import run
    m = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError):
        run([m, m], [], nc=4)
    with pytest.raises(ValueError):
        run([m, m], [], nc=4, wbf=dict(iou_thr=0.67), compute_loss=lambda p, t: (None, torch.zeros(3)))
    with pytest.raises(ValueError):
        run(m, [], nc=4, wbf={}, compute_loss=lambda p, t: (None, torch.zeros(3)))


def test_capacity_is_refused_before_any_launch():
    from dmayolo.utils.wbf import max_rows, wbf_padded, weighted_boxes_fusion
    cap = max_rows()
    assert cap >= 8 * 300  # the documented floor: 8 models x 300 rows
    M, R = 8, cap // 8 + 1
    with pytest.raises(NotImplementedError):  # host tensors: the refusal comes before anything touches a device
        wbf_padded(torch.zeros(M, 1, R, 6), torch.zeros(M, 1, dtype=torch.int32), torch.ones(1, 2))
    n = cap + 1
    with pytest.raises(NotImplementedError):
        weighted_boxes_fusion([np.zeros((n, 4), np.float32)], [np.zeros(n, np.float32)], [np.zeros(n, np.float32)])
