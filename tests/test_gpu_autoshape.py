"""GPU: AutoShape on the HIP path (models/common.py:701-891) -- the letterbox kernel (dmy_letterbox_batch) bit for bit
against data.letterbox on the host + Model.to_input, the box kernel (dmy_scale_boxes) bit for bit against scale_coords
+ xyxy2xywh + the gn divisions, the wrapper end to end against the same steps taken by hand, and its input forms.

The torch side of every box check runs on CPU fp32 copies: there `coords /= gain` divides (IEEE), which is what the
kernel does; on the GPU torch multiplies by the scalar's reciprocal, which differs in the last bit."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'dma-yolo_amd', 'dmayolo', 'configs', 'yolov5n.yaml')
# long side == size (no resize) / upscaled / portrait, downscaled, left-right border / odd border total (top != bottom)
SHAPES = [(48, 64), (37, 53), (150, 97), (33, 64)]
WIDE = [(60, 96), (30, 50)]  # landscape only: shape1 = 64 x 96 at size 96


def _images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


@functools.lru_cache(maxsize=None)
def _model(dtype):
    """yolov5n with 3 classes and seeded random weights; the objectness biases are raised so that a 64-pixel image of
    noise yields detections at conf 0.001 (the end-to-end tests assert that it does)"""
    from dmayolo.models.yolo import Model
    torch.manual_seed(7)
    m = Model(CFG, nc=3, act_dtype=dtype)
    det = m.model[-1]
    with torch.no_grad():
        for mi in det.m:
            mi.bias.view(det.na, -1)[:, 4] += 4.0
    return m.cuda().eval()


def _nchw(y):
    """the stem input as stored -> (NCHW image part, padding channels)"""
    if getattr(y, '_dmy_s2d', 0):
        N, Cs, H2, W2 = y.shape
        img = y[:, :12].reshape(N, 2, 2, 3, H2, W2).permute(0, 3, 4, 1, 5, 2).reshape(N, 3, 2 * H2, 2 * W2)
        return img, y[:, 12:]
    base = y._base if y._base is not None else y
    return y, base[:, 3:]


@pytest.mark.parametrize('shapes,size,want', [(SHAPES, 64, [64, 64]), (WIDE, 96, [64, 96])])
def test_letterbox_kernel_equals_host_letterbox(shapes, size, want):
    from dmayolo.data import letterbox
    from dmayolo.models.common import autoshape_geometry, letterbox_batch
    imgs = _images(shapes, 11)
    shape1, geo = autoshape_geometry(shapes, size, 32)
    assert shape1 == want
    if shapes is SHAPES:
        assert geo[0][:2] == (48, 64) and geo[1][0] > 37 and geo[2][:2] == (64, 41) and geo[2][3] > 0
        assert geo[3][2] == 15 and shape1[0] - geo[3][0] - geo[3][2] == 16
    host = np.stack([letterbox(im, new_shape=shape1, auto=False)[0] for im in imgs])
    xu = torch.from_numpy(host).permute(0, 3, 1, 2).cuda()
    flipped = [np.ascontiguousarray(im[:, :, ::-1]) for im in imgs]
    m = _model(torch.float32)
    keep = m.act_dtype, getattr(m, 's2d_stem', True)
    try:
        for dtype in (torch.float32, torch.bfloat16):
            for s2d in (True, False):
                m.act_dtype, m.s2d_stem = dtype, s2d
                ref = m.to_input(xu)
                tag = (dtype, s2d)
                assert bool(getattr(ref, '_dmy_s2d', 0)) == s2d, tag
                for src, swap in ((imgs, False), (flipped, True)):
                    got = letterbox_batch(src, shape1, geo, dtype, s2d, torch.device('cuda'), swap=swap)
                    assert got.dtype == dtype and got.shape == ref.shape and got.stride() == ref.stride(), tag
                    assert getattr(got, '_dmy_s2d', 0) == getattr(ref, '_dmy_s2d', 0), tag
                    assert getattr(got, '_dmy_cpad', 0) == getattr(ref, '_dmy_cpad', 0), tag
                    gi, gp = _nchw(got)
                    ri, rp = _nchw(ref)
                    assert torch.equal(gi, ri), (tag, swap, int((gi != ri).sum()))
                    assert not bool(gp.any()), tag  # zero channels past the image's
                    if not s2d:
                        assert gp.shape[1] == (1 if dtype == torch.float32 else 5)
                    border = (torch.tensor(114.0) * torch.tensor(1.0 / 255.0)).to(dtype).cuda()
                    for k, (h, w, top, left, _, _) in enumerate(geo):
                        mask = torch.ones(shape1, dtype=torch.bool, device='cuda')
                        mask[top:top + h, left:left + w] = False
                        assert bool((gi[k][:, mask] == border).all()), (tag, k)
    finally:
        m.act_dtype, m.s2d_stem = keep


def test_letterbox_kernel_refuses_bad_geometry():
    from dmayolo._lib import call, ptr, stream
    from dmayolo.models.common import LETTERBOX_DESC
    src = torch.zeros((4, 4, 3), dtype=torch.uint8, device='cuda')
    tab = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 3], [2048] * 4, [0] * 4], dtype=torch.int32, device='cuda')
    y = torch.zeros(8 * 8 * 16, dtype=torch.float32, device='cuda')

    def run(OH, OW, s2d, Cs, top=0, left=0, dtype=0):
        d = np.zeros(1, dtype=LETTERBOX_DESC)
        d['src'], d['xt'], d['yt'] = src.data_ptr(), tab.data_ptr(), tab.data_ptr()
        d['H0'] = d['W0'] = d['h'] = d['w'] = 4
        d['top'], d['left'] = top, left
        dd = torch.from_numpy(d.view(np.uint8)).cuda()
        call('dmy_letterbox_batch', dtype, ptr(dd), d.ctypes.data, 1, ptr(y), OH, OW, s2d, Cs, 1.0, stream())
        torch.cuda.synchronize()

    run(8, 8, 1, 12)
    run(7, 5, 0, 4, top=3, left=1)
    for bad in (dict(OH=7, OW=8, s2d=1, Cs=12), dict(OH=8, OW=7, s2d=1, Cs=12), dict(OH=8, OW=8, s2d=1, Cs=12, top=5),
                dict(OH=8, OW=8, s2d=0, Cs=4, left=5), dict(OH=8, OW=8, s2d=0, Cs=4, top=-1),
                dict(OH=8, OW=8, s2d=0, Cs=6), dict(OH=8, OW=8, s2d=1, Cs=12, dtype=1), dict(OH=8, OW=8, s2d=1, Cs=8)):
        with pytest.raises(RuntimeError, match='dmy_letterbox_batch failed with hipError 1'):
            run(**bad)


def test_scale_boxes_kernel_equals_scale_coords():
    from dmayolo.models.common import autoshape_geometry, scale_boxes
    from dmayolo.utils.general import scale_coords, xyxy2xywh
    shapes = [(48, 64), (150, 97), (37, 53)]
    shape1, geo = autoshape_geometry(shapes, 64, 32)
    assert len({g[4] for g in geo}) == 3  # three gains
    max_det, counts = 40, [33, 0, 40]
    g = torch.Generator().manual_seed(5)
    out = torch.rand((3, max_det, 6), generator=g) * 100.0 - 20.0  # canvas is 64 x 64: boxes leave it on every side
    out[0, :4, :4] = torch.tensor([[-5.0, 10.0, 30.0, 20.0], [10.0, -5.0, 30.0, 20.0], [10.0, 10.0, 90.0, 20.0],
                                   [10.0, 10.0, 30.0, 90.0]])
    before = out.clone()
    dev = out.cuda()
    xywh, xyxyn, xywhn = scale_boxes(dev, counts, geo, shapes)
    got = [t.cpu() for t in (dev, xywh, xyxyn, xywhn)]
    for b, (n, (h0, w0)) in enumerate(zip(counts, shapes)):
        ref = scale_coords(shape1, before[b, :n].clone(), (h0, w0))
        gn = torch.tensor([w0, h0, w0, h0, 1, 1])
        rwh = xyxy2xywh(ref)
        for name, t, r in (('xyxy', got[0], ref), ('xywh', got[1], rwh), ('xyxyn', got[2], ref / gn),
                           ('xywhn', got[3], rwh / gn)):
            assert torch.equal(t[b, :n], r), (b, name, float((t[b, :n] - r).abs().max()) if n else 0)
        assert torch.equal(got[0][b, n:], before[b, n:]), b  # rows past the count are not touched
    ref0 = scale_coords(shape1, before[0, :4].clone(), shapes[0])
    assert ref0[0, 0] == 0 and ref0[1, 1] == 0 and ref0[2, 2] == 64 and ref0[3, 3] == 48  # every side clamps


def _by_hand(m, imgs, size, augment, conf):
    from dmayolo.data import letterbox
    from dmayolo.models.common import autoshape_geometry
    from dmayolo.utils.general import non_max_suppression, scale_coords
    shape1, _ = autoshape_geometry([im.shape[:2] for im in imgs], size, 32)
    x = np.stack([letterbox(im, new_shape=shape1, auto=False)[0] for im in imgs])
    x = torch.from_numpy(np.ascontiguousarray(x.transpose((0, 3, 1, 2)))).cuda()
    with torch.no_grad():
        y = m(x, augment)[0]
    pred = non_max_suppression(y, conf, 0.45, classes=None, multi_label=False, max_det=1000)
    return [scale_coords(shape1, p.cpu().clone(), im.shape[:2]) for p, im in zip(pred, imgs)], shape1


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_autoshape_equals_hand_made_path(dtype, augment):
    from dmayolo.models.common import AutoShape, Detections
    from dmayolo.utils.general import xyxy2xywh
    m = _model(dtype)
    imgs = _images(SHAPES, 3)
    ref, shape1 = _by_hand(m, imgs, 64, augment, 0.001)
    assert all(r.shape[0] >= 1 for r in ref), [r.shape[0] for r in ref]  # else the comparison below is vacuous
    a = AutoShape(m)
    a.conf = 0.001
    d = a(list(imgs), size=64, augment=augment)
    assert isinstance(d, Detections) and d.n == len(d) == 4 and tuple(d.s) == (4, 3, *shape1)
    assert d.files == [f'image{i}.jpg' for i in range(4)] and d.names == m.names and len(d.t) == 3
    for i, r in enumerate(ref):
        assert d.pred[i].is_cuda and torch.equal(d.pred[i].cpu(), r), (i, d.pred[i].shape, r.shape)
        assert d.imgs[i].shape == imgs[i].shape and np.array_equal(d.imgs[i], imgs[i])
        gn = torch.tensor([imgs[i].shape[1], imgs[i].shape[0]] * 2 + [1, 1])
        assert torch.equal(d.xywh[i].cpu(), xyxy2xywh(r)) and torch.equal(d.xyxyn[i].cpu(), r / gn)
        assert torch.equal(d.xywhn[i].cpu(), xyxy2xywh(r) / gn)
    one = d.tolist()[2]
    assert one.n == 1 and one.files == ['image2.jpg'] and torch.equal(one.xyxy.cpu(), ref[2])


def test_autoshape_input_forms(tmp_path):
    from PIL import Image
    from dmayolo.models.common import AutoShape
    m = _model(torch.float32)
    a = m.autoshape()
    assert a.autoshape() is a and isinstance(a, AutoShape)
    a.conf = 0.001
    rng = np.random.default_rng(9)
    im = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    base = a(im, size=64)
    assert base.n == 1 and len(base.pred) == 1 and base.pred[0].shape[0] >= 1 and tuple(base.s) == (1, 3, 64, 64)
    Image.fromarray(im).save(tmp_path / 'img.png')
    rgba = np.concatenate([im, rng.integers(0, 256, (40, 56, 1), dtype=np.uint8)], 2)
    forms = {'chw': im.transpose(2, 0, 1), 'rgba': rgba, 'pil': Image.fromarray(im), 'str': str(tmp_path / 'img.png'),
             'path': tmp_path / 'img.png', 'list': [im]}
    for name, v in forms.items():
        d = a(v, size=64)
        assert d.n == 1 and torch.equal(d.pred[0], base.pred[0]), name
        assert np.array_equal(d.imgs[0], im), name
    assert a(str(tmp_path / 'img.png'), size=64).files == ['img.jpg']
    g3 = a(np.tile(grey[..., None], 3), size=64)
    assert g3.pred[0].shape[0] >= 1 and torch.equal(a(grey, size=64).pred[0], g3.pred[0])
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = m(x.cuda())
    got = a(x)
    assert torch.equal(got[0], want[0]) and all(torch.equal(p, q) for p, q in zip(got[1], want[1]))
    with pytest.raises(NotImplementedError):
        a('http://example.invalid/zidane.jpg', size=64)
    with pytest.raises(TypeError):
        a(im.astype(np.float32), size=64)
