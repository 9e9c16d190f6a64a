"""CPU: the IoU-kind additions to the C ABI and their Python front (no GPU, no launch).

The three entries are bound and exported (test_abi.py then compares their types with the header by itself), the kind
codes agree between the header and dmayolo._lib, ComputeLoss validates iou_type in its constructor, bbox_iou refuses
what the kernel cannot do, and its keywords map to kind codes with the reference's precedence
(utils/metrics.py:216-252)."""
import ctypes
import itertools
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dmy_yolo_loss_level_iou', 'dmy_yolo_loss_level_focal_iou', 'dmy_bbox_iou_eval']


def _model(**hyp):
    det = types.SimpleNamespace(nl=3, na=3, nc=10, anchors=torch.ones(3, 3, 2), stride=torch.tensor([8., 16., 32.]))
    return types.SimpleNamespace(hyp=dict(fl_gamma=0.0, **hyp), model=[det])


def test_new_entries_bound_and_exported():
    from dmayolo import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the _iou entries are the old ones plus a trailing int
    I = ctypes.c_int
    assert _lib.SIGNATURES['dmy_yolo_loss_level_iou'] == _lib.SIGNATURES['dmy_yolo_loss_level'] + [I]
    assert _lib.SIGNATURES['dmy_yolo_loss_level_focal_iou'] == _lib.SIGNATURES['dmy_yolo_loss_level_focal'] + [I]
    for old in ('dmy_yolo_loss_level', 'dmy_yolo_loss_level_focal', 'dmy_siou_eval'):
        assert old in _lib.SIGNATURES and hasattr(lib, old), old


def test_kind_codes_match_header():
    from dmayolo import _lib
    src = open(os.path.join(ROOT, 'include', 'dmayolo.h')).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define DMY_IOU_(\w+)\s+(\d+)', src, re.M)}
    assert codes == {'SIOU': 0, 'CIOU': 1, 'DIOU': 2, 'GIOU': 3, 'PLAIN': 4}
    assert _lib.IOU_KIND == {'siou': 0, 'ciou': 1, 'diou': 2, 'giou': 3, 'iou': 4}


def test_unknown_kind_is_refused_without_a_launch():
    """hipErrorInvalidValue (1) for a kind outside the table; with n = 0 and null pointers a launch would be an error
    of another kind, and a valid kind with n = 0 returns success without touching anything"""
    from dmayolo import _lib
    for kind in (-1, 5, 99):
        assert _lib.lib.dmy_bbox_iou_eval(kind, 0, None, None, None, None, 0, None) == 1
    for kind in range(5):
        assert _lib.lib.dmy_bbox_iou_eval(kind, 1, None, None, None, None, 0, None) == 0
    # the level entries: dtype 0, every size 0, every pointer null, then the kind -- refused before the first enqueue
    zero = {ctypes.c_void_p: None, ctypes.c_int: 0, ctypes.c_long: 0, ctypes.c_float: 0.0}
    bal = (ctypes.c_double * 8)(*([1.0] * 8))
    for name in ('dmy_yolo_loss_level_iou', 'dmy_yolo_loss_level_focal_iou'):
        args = [zero[t] for t in _lib.SIGNATURES[name][:-1]]
        if name.endswith('focal_iou'):
            assert _lib.SIGNATURES[name][19] is ctypes.c_void_p
            args[19] = ctypes.addressof(bal)  # balance: the focal entry refuses a null one before it looks at the kind
        for kind in (-1, 5):
            assert getattr(_lib.lib, name)(*args, kind) == 1, (name, kind)


def test_compute_loss_iou_type():
    from dmayolo.utils.loss import ComputeLoss
    assert ComputeLoss(_model()).iou_type == 'siou' and ComputeLoss(_model()).iou_kind == 0
    for name, code in [('siou', 0), ('ciou', 1), ('diou', 2), ('giou', 3), ('iou', 4), ('CIoU', 1), ('GIOU', 3)]:
        cl = ComputeLoss(_model(), iou_type=name)
        assert cl.iou_kind == code and cl.iou_type == name.lower()
    assert ComputeLoss(_model(iou_type='DIoU')).iou_kind == 2          # the hyp key
    assert ComputeLoss(_model(iou_type='diou'), iou_type='giou').iou_kind == 3  # the argument wins
    assert ComputeLoss(_model(), autobalance=True, iou_type='ciou').autobalance
    for bad in ('eiou', '', 'siou ', 3):
        with pytest.raises(ValueError):
            ComputeLoss(_model(), iou_type=bad)
    with pytest.raises(ValueError):
        ComputeLoss(_model(iou_type='alpha'))


def test_bbox_iou_refusals_on_cpu():
    from dmayolo.utils.metrics import bbox_iou
    b1, b2 = torch.rand(4, 5), torch.rand(5, 4)
    with pytest.raises(NotImplementedError):
        bbox_iou(b1, b2)
    with pytest.raises(NotImplementedError):
        bbox_iou(b1[:, 0], b2, x1y1x2y2=False, CIoU=True)


def test_flag_precedence():
    """SIoU before everything, DIoU before CIoU (the reference tests `if DIoU` first inside `elif CIoU or DIoU`),
    GIoU only when none of the three is set"""
    from dmayolo.utils.metrics import iou_kind
    S, C, D, G, P = 0, 1, 2, 3, 4
    for g, d, c, s in itertools.product([False, True], repeat=4):
        want = S if s else D if d else C if c else G if g else P
        assert iou_kind(GIoU=g, DIoU=d, CIoU=c, SIoU=s) == want, (g, d, c, s)
    assert iou_kind() == P and iou_kind(GIoU=True) == G and iou_kind(GIoU=True, CIoU=True) == C
    assert iou_kind(CIoU=True, DIoU=True) == D and iou_kind(GIoU=True, DIoU=True, CIoU=True, SIoU=True) == S
