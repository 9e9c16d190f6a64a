"""CPU: the host plan of the test-time-augmented forward (models/yolo.py tta_plan) against values worked by hand from
the reference's formulas (models/yolo.py:194-209, 266-275; utils/torch_utils.py:264-274):
resized = int(size * ratio), padded = ceil(size * ratio / gs) * gs, and _clip_augmented's index formula."""
import pytest


def _levels(strides):
    return lambda hp, wp: [(hp // s, wp // s) for s in strides]


def _plan(h, w, strides=(8, 16, 32), na=3):
    from dmayolo.models.yolo import tta_plan
    return tta_plan(h, w, max(strides), _levels(strides), na)


def test_pass_list_is_the_six_pass_fork():
    passes, _ = _plan(64, 64)
    assert [p[0] for p in passes] == [1, 1, 0.83, 0.83, 0.67, 0.67]
    assert [p[1] for p in passes] == [0, 3, 0, 3, 0, 3]


@pytest.mark.parametrize('size,resized,padded', [(640, (531, 428), (544, 448)), (1536, (1274, 1029), (1280, 1056))])
def test_square_sizes(size, resized, padded):
    passes, _ = _plan(size, size)
    for k in (0, 1):
        assert passes[k][2] == (size, size) and passes[k][3] == (size, size)
    for k, r, p in ((2, resized[0], padded[0]), (3, resized[0], padded[0]), (4, resized[1], padded[1]),
                    (5, resized[1], padded[1])):
        assert passes[k][2] == (r, r) and passes[k][3] == (p, p), (k, passes[k])


def test_non_square_96x160():
    passes, total = _plan(96, 160)
    assert passes[2][2:4] == ((79, 132), (96, 160)) and passes[3][2:4] == ((79, 132), (96, 160))
    assert passes[4][2:4] == ((64, 107), (96, 128)) and passes[5][2:4] == ((64, 107), (96, 128))
    full, small = 3 * (12 * 20 + 6 * 10 + 3 * 5), 3 * (12 * 16 + 6 * 8 + 3 * 4)
    assert total == 4 * full + 2 * small - 3 * 3 * 5 - 3 * 12 * 16


def test_64_nl3_rows_masks_offsets():
    passes, total = _plan(64, 64)
    assert total == 1308  # 6 * 252 - 12 - 192
    assert [p[4] for p in passes] == [0b011, 0b111, 0b111, 0b111, 0b111, 0b110]
    assert [p[5] for p in passes] == [0, 240, 492, 744, 996, 1248]


def test_four_levels_drop_the_right_ones():
    passes, total = _plan(64, 64, strides=(4, 8, 16, 32))
    per = [3 * (64 // s) ** 2 for s in (4, 8, 16, 32)]  # 768, 192, 48, 12
    assert [p[4] for p in passes] == [0b0111, 0b1111, 0b1111, 0b1111, 0b1111, 0b1110]
    assert total == 6 * sum(per) - per[3] - per[0]
    assert passes[1][5] == sum(per) - per[3] and passes[5][5] == total - (sum(per) - per[0])


@pytest.mark.parametrize('h,w', [(100, 64), (64, 100), (650, 650)])
def test_size_not_a_stride_multiple_raises(h, w):
    with pytest.raises(ValueError):
        _plan(h, w)
