"""CPU: the numpy restatement of the confusion-matrix matching (tests/confusion_ref.py) reproduces the matrices that
the reference's own ConfusionMatrix.process_batch (utils/metrics.py:122-160) gave for the recorded inputs
(tests/golden/confusion_*.npz), exactly, and the hand-derived answers; the new C-ABI entry is declared, bound and
exported.  Everything is integer equality: the IoUs are fp32 bit patterns and the counters integers."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confusion_cases as cases  # noqa: E402
import confusion_ref as ref  # noqa: E402


def test_goldens_present():
    assert len(cases.GOLDEN) >= 3


@pytest.mark.parametrize('path', cases.GOLDEN, ids=os.path.basename)
def test_golden_ious_are_distinct(path):
    """the fixture condition: within every image all IoUs above the threshold are pairwise distinct in fp32, so the
    recorded matrix does not depend on how the reference's sorts order exact ties"""
    dets, labs, nc, conf, thr, want = cases.load_golden(path)
    assert all(ref.distinct_ious(d, l, conf, thr) for d, l in zip(dets, labs))
    assert want.shape == (nc + 1, nc + 1) and want.sum() > 0


@pytest.mark.parametrize('path', cases.GOLDEN, ids=os.path.basename)
def test_restatement_reproduces_reference_matrix(path):
    dets, labs, nc, conf, thr, want = cases.load_golden(path)
    got = ref.confusion_matrix(dets, labs, nc, conf, thr)
    assert np.array_equal(got, want), np.argwhere(got != want)


def test_goldens_cover_the_rules():
    """the recorded images do exercise what the matching is about: more than 16 candidates in one image, a detection
    that loses its best label, unmatched labels, and a confidence equal to the threshold"""
    many = lost = unmatched = at_conf = 0
    for path in cases.GOLDEN:
        dets, labs, nc, conf, thr, _ = cases.load_golden(path)
        for d, l in zip(dets, labs):
            kept, lab_det = ref.match(d, l, conf, thr)
            iou = ref.box_iou(l[:, 1:], d[kept, :4])
            many += int((iou > np.float32(thr)).sum() > 16)
            cand = (iou > np.float32(thr)).any(0)
            lost += int(cand.sum() - (lab_det >= 0).sum())
            unmatched += int((lab_det < 0).sum())
            at_conf += int((d[:, 4] == np.float32(conf)).sum())
    assert many >= 3 and lost >= 10 and unmatched >= 10 and at_conf >= 1, (many, lost, unmatched, at_conf)


@pytest.mark.parametrize('name', sorted(cases.HAND))
def test_restatement_hand_cases(name):
    dets, labs, nc, conf, thr, cells = cases.HAND[name]
    d, l = cases.arrays(dets, labs)
    assert np.array_equal(ref.confusion_matrix([d], [l], nc, conf, thr), cases.dense(nc, cells))


def test_restatement_drops_out_of_range_classes():
    dets, labs, nc, conf, thr, cells = cases.OUT_OF_RANGE
    d, l = cases.arrays(dets, labs)
    assert np.array_equal(ref.confusion_matrix([d], [l], nc, conf, thr), cases.dense(nc, cells))


def test_abi_entry_declared_bound_and_exported():
    """include/dmayolo.h declares dmy_confusion_matrix, csrc/metrics.hip defines it, dmayolo/_lib.py binds it with the
    header's types and the library exports it (what tests/test_abi.py checks for every symbol)"""
    from test_abi import CSRC, header_decls
    from dmayolo import _lib
    decls = header_decls()
    assert 'dmy_confusion_matrix' in decls
    ret, args = decls['dmy_confusion_matrix']
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert ret is I and args == [P, P, P, P, I, I, F, F, P, P, P, P, P, P]
    assert _lib.SIGNATURES['dmy_confusion_matrix'] == args
    assert 'DMY_API int dmy_confusion_matrix(' in open(os.path.join(CSRC, 'metrics.hip')).read()
    fn = getattr(ctypes.CDLL(_lib.LIB_PATH), 'dmy_confusion_matrix')
    assert fn is not None and _lib.lib.dmy_confusion_matrix.restype is I


def test_confusion_matrix_class_interface():
    """constructor attributes and the empty matrix need no GPU; a CPU tensor is refused, never computed elsewhere"""
    import torch
    from dmayolo.utils.metrics import ConfusionMatrix
    cm = ConfusionMatrix(4)
    assert (cm.nc, cm.conf, cm.iou_thres) == (4, 0.25, 0.45)
    m = cm.matrix
    assert m.shape == (5, 5) and m.dtype == np.float64 and not m.any()
    assert (ConfusionMatrix(2, conf=0.1, iou_thres=0.6).conf, ConfusionMatrix(2, 0.1, 0.6).iou_thres) == (0.1, 0.6)
    with pytest.raises(RuntimeError, match='GPU'):
        cm.process_batch(torch.zeros(1, 6), torch.zeros(1, 5))


def test_print_writes_one_line_per_row(capsys):
    from dmayolo.utils.metrics import ConfusionMatrix
    cm = ConfusionMatrix(2)
    cm.print()
    out = capsys.readouterr().out.splitlines()
    assert out == [' '.join(map(str, np.zeros(3)))] * 3


def test_plot_never_raises(tmp_path, capsys):
    """a missing plotting library is a printed warning (utils/metrics.py:184-185); with one, the file is written"""
    from dmayolo.utils.metrics import ConfusionMatrix
    ConfusionMatrix(2).plot(save_dir=str(tmp_path), names=['a', 'b'])
    out = capsys.readouterr().out
    assert (tmp_path / 'confusion_matrix.png').exists() or 'WARNING: ConfusionMatrix plot failure' in out
