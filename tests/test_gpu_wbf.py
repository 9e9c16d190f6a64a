"""Weighted boxes fusion on the gfx950 kernels (csrc/wbf.hip) against the host restatement (tests/wbf_ref.py), bit for
bit; the library-signature wrapper; val.run over a list of models; Ensemble / attempt_load with a list of files."""
import os

import numpy as np
import pytest
import torch

from test_wbf_ref import CASES
from wbf_ref import wbf_image, wbf_padded_ref, weighted_boxes_fusion_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'dma-yolo_amd', 'dmayolo', 'configs', 'yolov5n.yaml')
M, NIMG, R = 3, 2, 64
WH = ((640, 480), (1536, 864))


def _iou64(a, b, W, H):
    """the restatement's IoU of two pixel boxes after its fp64 normalisation"""
    a = [float(np.float32(a[0])) / W, float(np.float32(a[1])) / H, float(np.float32(a[2])) / W,
         float(np.float32(a[3])) / H]
    b = [float(np.float32(b[0])) / W, float(np.float32(b[1])) / H, float(np.float32(b[2])) / W,
         float(np.float32(b[3])) / H]
    inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _make_input():
    """(dets [M, NIMG, R, 6], counts [M, NIMG]): jittered groups around 12 shared centres per image (labels 0-2) plus
    the planted rows: score ties, IoU exactly at the threshold, rows outside the image, degenerate and swapped rows,
    a cluster of more than M members, a label of one model only, an empty (model, image), output-score ties"""
    rng = np.random.RandomState(11)
    rows = [[[] for _ in range(NIMG)] for _ in range(M)]
    for b, (W, H) in enumerate(WH):
        cen = np.stack([rng.uniform(0.1, 0.9, 12) * W, rng.uniform(0.1, 0.9, 12) * H], 1)
        size = np.stack([rng.uniform(0.05, 0.25, 12) * W, rng.uniform(0.05, 0.25, 12) * H], 1)
        lab = rng.randint(0, 3, 12)
        for t in range(M):
            for k in range(12):
                for _ in range(rng.randint(0, 3)):  # 0-2 detections of this centre by this model
                    c = cen[k] + rng.randn(2) * 0.03 * size[k]
                    s = size[k] * (1 + 0.03 * rng.randn(2))
                    rows[t][b].append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2,
                                       rng.uniform(0.005, 0.95), lab[k]])  # some scores are under skip_box_thr 0.01
            # one cluster with more than M members: centre 0, 3 near-identical rows per model
            for _ in range(3):
                c = cen[0] + rng.randn(2) * 0.004 * size[0]
                rows[t][b].append([c[0] - size[0, 0] / 2, c[1] - size[0, 1] / 2, c[0] + size[0, 0] / 2,
                                   c[1] + size[0, 1] / 2, rng.uniform(0.3, 0.9), lab[0]])
            # exact score ties across models (0.5 in every model, same cluster) and within a model (0.625 twice)
            for sc in (0.5, 0.625, 0.625):
                c = cen[1] + rng.randn(2) * 0.02 * size[1]
                rows[t][b].append([c[0] - size[1, 0] / 2, c[1] - size[1, 1] / 2, c[0] + size[1, 0] / 2,
                                   c[1] + size[1, 1] / 2, sc, lab[1]])
            # rows reaching outside the image, a row wholly outside it and a zero-size row (both degenerate after the
            # clamp), a row given with x2 < x1 and y2 < y1
            rows[t][b].append([-0.1 * W, 0.2 * H, 0.2 * W, 0.5 * H, 0.7, 1])
            rows[t][b].append([0.8 * W, 0.7 * H, 1.2 * W, 1.3 * H, 0.6, 2])
            rows[t][b].append([1.1 * W, 0.1 * H, 1.3 * W, 0.3 * H, 0.8, 0])
            rows[t][b].append([0.3 * W, 0.3 * H, 0.3 * W, 0.6 * H, 0.8, 0])
            rows[t][b].append([0.7 * W, 0.6 * H, 0.5 * W, 0.4 * H, 0.4 + 0.1 * t, 2])
        # lone rows of one score: their clusters tie in the output order, within a label and across labels
        rows[0][b] += [[10, 10, 30, 30, 0.375, 0], [600, 440, 630, 470, 0.375, 0], [10, 440, 30, 470, 0.375, 1]]
    # label 3 lives in model 0 only; image 0 holds one pair at IoU exactly 0.55 and one at exactly 0.67 (the second box
    # of each pair meets its partner's still unfused cluster: the scores order the four rows A, A', B, B')
    W, H = WH[0]
    pairs = {0.55: ([0, 0, 80, 240], [0, 0, 44, 240]), 0.67: ([32, 0, 132, 240], [32, 0, 99, 240])}
    for thr, (A, B) in pairs.items():
        assert _iou64(A, B, W, H) == thr
    rows[0][0] += [pairs[0.55][0] + [0.9, 3], pairs[0.67][0] + [0.89, 3], pairs[0.55][1] + [0.5, 3],
                   pairs[0.67][1] + [0.49, 3]]
    rows[0][1] += [[100, 100, 400, 300, 0.75, 3], [110, 95, 405, 310, 0.7, 3]]
    rows[1][1] = []  # counts of 0 for one (model, image)
    dets = rng.uniform(0.2, 0.9, (M, NIMG, R, 6)).astype(np.float32) * np.float32([300, 200, 600, 400, 1, 3])  # past the
    counts = np.zeros((M, NIMG), np.int32)  # counts: plausible rows that must never be read
    for t in range(M):
        for b in range(NIMG):
            r = np.asarray(rows[t][b], np.float32).reshape(-1, 6)
            r = r[rng.permutation(len(r))]
            assert len(r) <= R
            dets[t, b, :len(r)] = r
            counts[t, b] = len(r)
    return dets, counts


_INPUT = {}


def _input(variant):
    """'full': both images populated; 'empty_image': image 1 has every count 0"""
    if not _INPUT:
        dets, counts = _make_input()
        empty = counts.copy()
        empty[:, 1] = 0
        _INPUT.update(full=(dets, counts), empty_image=(dets, empty))
    return _INPUT[variant]


_REF = {}


def _ref(variant, weights, thr):
    key = (variant, weights, thr)
    if key not in _REF:
        dets, counts = _input(variant)
        _REF[key] = wbf_padded_ref(dets, counts, WH, weights, *thr)
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('variant', ['full', 'empty_image'])
@pytest.mark.parametrize('weights', [None, (2, 1, 1)])
@pytest.mark.parametrize('thr', [(0.55, 0.0), (0.67, 0.01)])
def test_kernel_matches_restatement_bit_for_bit(variant, weights, thr):
    from dmayolo.utils.wbf import wbf_padded
    dets, counts = _input(variant)
    want = _ref(variant, weights, thr)
    out, res = wbf_padded(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(),
                          torch.tensor(WH, dtype=torch.float32).cuda(), weights, *thr)
    assert out.shape == (NIMG, M * R, 6) and len(res) == NIMG
    print([len(w) for w in want], [len(r) for r in res])
    for b in range(NIMG):
        got = res[b].cpu().numpy()
        assert got.shape == want[b].shape, (b, got.shape, want[b].shape)
        diff = np.argwhere(_bits(got) != _bits(want[b]))
        assert len(diff) == 0, (b, diff[:8], got[diff[:4, 0]], want[b][diff[:4, 0]])
    # the input does what it was built for: clusters form (fewer outputs than records) and image 1 can be empty
    assert 0 < len(want[0]) < counts[:, 0].sum() // 2
    assert (len(want[1]) == 0) == (variant == 'empty_image')
    assert len(np.unique(want[0][:, 4])) <= len(want[0]) - 2  # output score ties
    assert 3 in want[0][:, 5] and 3 in _ref('full', weights, thr)[1][:, 5]


def test_more_clusters_than_threads_in_one_label():
    """320 clusters of one label: the cluster block's 256 threads each hold more than one cluster in the IoU pass, and
    the best one lies in any wave"""
    from dmayolo.utils.wbf import wbf_padded
    rng = np.random.RandomState(5)
    W, H, n = 1280, 1024, 320
    gx, gy = np.meshgrid(np.arange(20) * 64 + 8, np.arange(16) * 64 + 8)
    base = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 48, gy.ravel() + 48], 1).astype(np.float64)
    dets = np.zeros((2, 1, n, 6), np.float32)
    for t in range(2):
        p = rng.permutation(n)
        dets[t, 0, :, :4] = base[p] + rng.randn(n, 4) * (1.5 * t)
        dets[t, 0, :, 4] = rng.uniform(0.05, 0.95, n)
    counts, wh = np.full((2, 1), n, np.int32), np.float32([[W, H]])
    want = wbf_padded_ref(dets, counts, wh, None, 0.55, 0.0)[0]
    assert 256 < len(want) < 2 * n - 256  # more clusters than threads, and most of them fused two rows
    got = wbf_padded(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(wh).cuda())[1][0]
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize('name', sorted(CASES))
def test_library_signature_on_device(name):
    from dmayolo.utils.wbf import weighted_boxes_fusion
    b, s, l, thr = CASES[name]
    want = weighted_boxes_fusion_ref(b, s, l, iou_thr=thr)
    got = weighted_boxes_fusion(b, s, l, iou_thr=thr)
    # lists, arrays and tensors are all taken
    got_t = weighted_boxes_fusion([torch.tensor(x, dtype=torch.float32).reshape(-1, 4) for x in b],
                                  [np.asarray(x, np.float32) for x in s], l, iou_thr=thr)
    for g in (got, got_t):
        assert all(isinstance(a, np.ndarray) for a in g)
        for a, w in zip(g, want):
            assert a.shape == w.shape and np.array_equal(_bits(a), _bits(w)), (name, a, w)


def _v5n(seed, nc=4):
    from dmayolo.models.yolo import Model
    torch.manual_seed(seed)
    m = Model(CFG, nc=nc)
    # a fresh Detect head scores everything near exp(bias) ~ 0.001, under any skip_box_thr: lift the objectness bias
    # and widen the head's weights so that scores spread over (0, 1) and boxes move with the image
    with torch.no_grad():
        for mi in m.model[-1].m:
            mi.weight *= 8
            mi.bias.view(m.model[-1].na, -1)[:, 4] += 4
    return m.cuda()


def test_val_run_with_model_list():
    from dmayolo.synthetic import targets as synthetic_targets
    from dmayolo.utils.general import non_max_suppression
    from dmayolo.val import batch_stats, run, summarize
    nc, S = 4, 64
    m0, m1 = _v5n(0), _v5n(1)
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (2, 3, S, S), generator=g, dtype=torch.uint8),
                synthetic_targets(2, nc, per_image=6, seed=3).cpu())]
    wbf = dict(iou_thr=0.67, skip_box_thr=0.01, weights=None)
    single_before = run(m0, batches, nc=nc)
    got = run([m0, m1], batches, nc=nc, wbf=wbf)
    assert m0.training and m1.training  # modes restored

    iouv = torch.linspace(0.5, 0.95, 10).cuda()
    stats, stats0 = [], []
    for img, targets in batches:
        img, targets = img.cuda(), targets.cuda().float()
        targets[:, 2:] *= S
        per_model = []
        for m in (m0, m1):
            m.eval()
            with torch.no_grad():
                per_model.append(non_max_suppression(m(img)[0], 0.001, 0.6, multi_label=True, max_det=300))
            m.train()
        fused = [torch.from_numpy(wbf_image([pm[b].cpu().numpy() for pm in per_model], S, S, None, 0.67, 0.01)).cuda()
                 for b in range(img.shape[0])]
        print([len(p) for pm in per_model for p in pm], [len(f) for f in fused])
        assert all(len(f) for f in fused)
        stats += batch_stats(fused, targets, (S, S), iouv)
        stats0 += batch_stats([p.clone() for p in per_model[0]], targets, (S, S), iouv)
    for (res, maps, seen, nt), st in ((got, stats), (single_before, stats0)):
        mp, mr, map50, map_, wmaps, wnt = summarize(st, nc)
        assert seen == 2 and res[:4] == (mp, mr, map50, map_) and res[4:] == (0.0, 0.0, 0.0)
        assert np.array_equal(maps, wmaps) and np.array_equal(nt, wnt)
    # a single model without wbf is the path it was, whatever ran in between
    again = run(m0, batches, nc=nc)
    assert again[0] == single_before[0] and np.array_equal(again[1], single_before[1])


def test_attempt_load_list_gives_ensemble(tmp_path):
    from dmayolo.models.yolo import Model
    from dmayolo.utils.ckpt import Ensemble, attempt_load, save_checkpoint
    paths = []
    for seed in (0, 1):
        paths.append(str(tmp_path / f'm{seed}.pt'))
        save_checkpoint(paths[-1], _v5n(seed))
    ens = attempt_load(paths)
    assert isinstance(ens, Ensemble) and len(ens) == 2 and not ens.training
    single = [attempt_load(p) for p in paths]
    assert all(type(m) is Model for m in single) and type(attempt_load(paths[:1])) is Model
    assert ens.names == single[-1].names and torch.equal(ens.stride, single[0].stride)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        y, train_out = ens(x)
        want = torch.cat([m(x)[0] for m in single], 1)
    assert train_out is None and y.shape[1] == 2 * single[0](x)[0].shape[1]
    assert torch.equal(y, want)
