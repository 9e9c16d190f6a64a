"""The conv plans' answers, pinned: dmy_conv_route (forward, data-grad, weight-grad), dmy_conv_fwd_bn_rows (without and
with a bias), dmy_conv_fwd_splitk_elems and dmy_conv_wgrad_ws_elems over every conv layer of the two bench
configurations and one geometry on each side of every branch of plan_fwd / plan_v3 / plan_dgrad / plan_wgrad, fp32 and
bf16.  The queries are host code: they read geometry, pointer alignment and the CU count (256 without a device, the
MI355X's own), so the fixture tests/golden/conv_routes.json holds on either machine.  An edit of the plans that moves
an answer shows here; one that means to regenerates the fixture:

    python tests/test_conv_routes.py          (DMY_LIB_AB=<other in-tree build> to record from that one)
"""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'conv_routes.json')
A, B, C_ = 1 << 30, 2 << 30, 3 << 30  # 16-byte aligned fake addresses: the queries only test alignment
NULL = -1  # a pointer offset that stands for a null pointer


def _geom(shape, N=None):
    """(N, C, H, W, K, k, s) in the SHAPES convention of test_gpu_conv.py -> the entries' 13 geometry scalars"""
    n, C, H, W, K, k, s = shape
    p = k // 2 if k != 6 else 2
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return [N or n, H, W, C, C, K, k, k, s, p, OH, OW, K]


def rows():
    """[geom (13), offsets of the three pointers (NULL = null), acc]: the model layers, then the edge geometries"""
    from test_gpu_conv_bench_shapes import DMA, V5S
    out = []
    # every conv layer of DMA-YOLO @1536 (batch 32, 1) and yolov5s @640 (batch 64, 1), with the space-to-depth k3 views
    # of their 6x6 image stems
    for shapes in (DMA + [(32, 16, 768, 768, 64, 3, 1)], V5S + [(64, 16, 320, 320, 32, 3, 1)]):
        for sh in shapes:
            for N in (sh[0], 1):
                out.append(_geom(sh, N) + [0, 0, 0, 0])
    # one base geometry per kernel kind, each perturbed along every axis of the 16-byte vector contract
    bases = [(2, 16, 20, 18, 24, 3, 1), (2, 1024, 48, 48, 1024, 3, 1), (64, 32, 320, 320, 64, 3, 2),
             (16, 64, 128, 128, 128, 3, 2), (32, 256, 192, 192, 512, 3, 2), (32, 64, 384, 384, 64, 3, 1),
             (32, 128, 192, 192, 512, 1, 1), (32, 512, 192, 192, 128, 1, 1), (32, 128, 192, 192, 128, 1, 1),
             (32, 512, 48, 48, 512, 1, 1), (32, 256, 96, 96, 256, 3, 1), (32, 128, 192, 192, 128, 3, 1),
             (12, 96, 37, 45, 136, 3, 1), (8, 16, 288, 288, 64, 3, 1), (16, 128, 40, 40, 256, 1, 1),
             (64, 128, 384, 384, 64, 1, 1), (64, 256, 384, 384, 64, 1, 1), (1, 256, 20, 20, 256, 3, 1)]
    for sh in bases:
        g = _geom(sh)
        out.append(g + [0, 0, 0, 1])  # accumulating data-grad
        for i in range(3):  # each base 2 bytes off 16-byte alignment, each base null
            off = [0, 0, 0]
            off[i] = 2
            out.append(g + off + [0])
            off[i] = NULL
            out.append(g + off + [0])
        for idx, d in ((4, 4), (12, 4), (4, 64), (12, 64)):  # x / y pixel stride: not a multiple of 8, a wider multiple
            h = list(g)
            h[idx] += d
            out.append(h + [0, 0, 0, 0])
        n, C, H, W, K, k, s = sh
        out.append(_geom((n, C + 4, H, W, K, k, s)) + [0, 0, 0, 0])  # C not a multiple of 8
        out.append(_geom((n, C + 8, H, W, K, k, s)) + [0, 0, 0, 0])  # C not a multiple of 64 (nor of 16 for C = 16)
    # M just under / at 16384 for every column count that changes the path
    for K in (24, 32, 64, 65, 72, 128, 256, 257, 264):
        for k in (1, 3):
            out.append(_geom((1, 64, 128, 128, K, k, 1)) + [0, 0, 0, 0])
            out.append(_geom((1, 64, 127, 129, K, k, 1)) + [0, 0, 0, 0])
            out.append(_geom((1, 256, 128, 128, K, k, 1)) + [0, 0, 0, 0])
    edges = [
        # halo: 256 / 248 tiles of 8 x 32 on 256 CUs, a height that is no multiple of 8, a width no multiple of 32
        (1, 64, 256, 256, 64, 3, 1), (1, 64, 248, 256, 64, 3, 1), (2, 64, 252, 256, 64, 3, 1), (2, 64, 256, 240, 64, 3, 1),
        # buffer descriptors: x and y extents at 2^32 bytes (past the limit) and just under
        (32, 64, 1024, 1024, 64, 3, 1), (31, 64, 1024, 1024, 64, 3, 1), (32, 64, 1024, 1024, 64, 1, 1),
        (32, 128, 1024, 1024, 32, 1, 1), (32, 32, 1024, 1024, 128, 1, 1), (16, 64, 2048, 1024, 128, 3, 2),
        # streaming 1x1 GEMM: K >= 2 C in whole 32-column groups, K = 2 C - 32, K % 32 != 0; its data-grad with 4 and 5
        # column groups
        (8, 64, 96, 96, 128, 1, 1), (8, 64, 96, 96, 160, 1, 1), (8, 64, 96, 96, 96, 1, 1), (8, 64, 96, 96, 136, 1, 1),
        (8, 256, 96, 96, 512, 1, 1), (8, 128, 96, 96, 256, 1, 1), (32, 1024, 96, 96, 256, 1, 1),
        (32, 1280, 96, 96, 256, 1, 1),
        # 16-channel 3x3 stem view: 32 / 64 / 256 / 288 / 48 columns
        (8, 16, 64, 64, 32, 3, 1), (8, 16, 64, 64, 64, 3, 1), (8, 16, 64, 64, 256, 3, 1), (8, 16, 64, 64, 288, 3, 1),
        (8, 16, 64, 64, 48, 3, 1),
        # persistent 1x1: 64 / 128 / 256 / 264 columns, one K step, 129..256 columns over 960 / 1024 channels
        (8, 64, 96, 96, 64, 1, 1), (8, 128, 96, 96, 64, 1, 1), (8, 256, 96, 96, 256, 1, 1), (8, 256, 96, 96, 264, 1, 1),
        (32, 960, 96, 96, 256, 1, 1), (32, 1024, 96, 96, 128, 1, 1),
        # wide tile: 256 / 255 tiles of 256 x 256; 288-row tiles; tall tile: 1024 / 1023 tiles of 512 x 128
        (16, 256, 64, 64, 256, 3, 1), (15, 256, 64, 68, 256, 3, 1), (32, 512, 96, 96, 512, 3, 1),
        (32, 128, 128, 128, 128, 3, 1), (31, 128, 128, 132, 128, 3, 1), (32, 128, 128, 128, 64, 3, 1),
        # split-K of small M: 3x3 with C % 64 == 0, its 1x1, C = 96, K = 24, a grid that already fills the chip
        (1, 256, 20, 20, 256, 3, 1), (1, 256, 20, 20, 256, 1, 1), (1, 96, 20, 20, 256, 3, 1), (1, 256, 20, 20, 24, 3, 1),
        (1, 64, 96, 96, 512, 3, 1), (1, 512, 40, 40, 45, 1, 1),
        # stride 2: odd extents, 256 / 240 tiles of 256 dy pixels, K % 64 != 0, 6x6, 1x1, 128 and 256 channels
        (12, 64, 75, 91, 128, 3, 2), (8, 128, 101, 99, 192, 3, 2), (16, 64, 128, 128, 64, 3, 2),
        (15, 64, 128, 128, 64, 3, 2), (16, 128, 128, 128, 128, 3, 2), (15, 128, 128, 128, 128, 3, 2),
        (16, 32, 128, 128, 64, 3, 2), (16, 64, 128, 128, 96, 3, 2), (8, 8, 192, 192, 64, 6, 2), (16, 64, 128, 128, 64, 1, 2),
        (16, 512, 96, 96, 512, 3, 2), (4, 64, 33, 35, 64, 3, 2),
        # register-staged data-grad: 4096 rows and 256 tiles of 128 x 128 at and under both limits
        (1, 128, 64, 64, 128, 3, 1), (1, 128, 63, 65, 128, 3, 1), (1, 1024, 64, 64, 64, 3, 1), (1, 64, 64, 64, 1024, 3, 1),
        # weight-grad: 10000 / 9984 tap units, the 8 M-pixel rule of 64 output channels with every column-tile case
        # (128 / 144 / 256 / 320 / 512 columns), 32 output channels, v4's 256 rows and 128 columns, 64 / 63 columns
        (5, 128, 160, 200, 128, 3, 1), (4, 128, 160, 200, 128, 3, 1), (64, 16, 384, 384, 64, 3, 1),
        (64, 144, 384, 384, 64, 1, 1), (64, 320, 384, 384, 64, 1, 1), (64, 512, 384, 384, 64, 1, 1),
        (63, 128, 360, 360, 64, 1, 1), (64, 128, 384, 384, 32, 1, 1), (16, 64, 40, 40, 256, 1, 1),
        (16, 128, 40, 40, 248, 1, 1), (16, 64, 40, 40, 128, 1, 1), (16, 56, 40, 40, 128, 1, 1), (16, 64, 40, 40, 64, 1, 1),
    ]
    out += [_geom(sh) + [0, 0, 0, 0] for sh in edges]
    # a stride-1 data-grad whose output extent is not the full convolution's
    g = _geom((32, 128, 64, 64, 128, 3, 1))
    g[10] -= 2
    out.append(g + [0, 0, 0, 0])
    return out


def answers(lib, row, dtype):
    """the seven pinned answers of one row"""
    g, (oa, ob, oc), acc = row[:13], row[13:16], row[16]
    a, b, c = (None if o == NULL else base + o for base, o in ((A, oa), (B, ob), (C_, oc)))
    bias = ctypes.cast(4 << 30, ctypes.POINTER(ctypes.c_float))
    return [lib.dmy_conv_route(0, dtype, a, b, c, *g, acc), lib.dmy_conv_route(1, dtype, a, b, c, *g, acc),
            lib.dmy_conv_route(2, dtype, a, b, c, *g, acc), lib.dmy_conv_fwd_bn_rows(dtype, a, b, None, c, *g),
            lib.dmy_conv_fwd_bn_rows(dtype, a, b, bias, c, *g), lib.dmy_conv_fwd_splitk_elems(dtype, a, b, c, *g),
            lib.dmy_conv_wgrad_ws_elems(dtype, a, b, *g, 0)]


def record(lib):
    return [row + answers(lib, row, 0) + answers(lib, row, 1) for row in rows()]


def test_conv_routes_match_fixture():
    from dmayolo import _lib
    want = json.load(open(FIXTURE))['rows']
    assert [w[:17] for w in want] == rows(), 'the fixture does not hold the geometry list of rows(): regenerate it'
    bad = [(w[:17], w[17:], got) for w in want for got in [answers(_lib.lib, w[:17], 0) + answers(_lib.lib, w[:17], 1)]
           if got != w[17:]]
    assert not bad, f'{len(bad)} of {len(want)} rows changed their plan, the first: {bad[:3]}'


def test_fixture_reaches_every_kernel_kind():
    """on the fixture's 256 CUs the rows reach every DMY_KERN_* code; SPLITK, which dmy_conv_route cannot answer (it has
    no workspace to offer), is pinned by rows whose dmy_conv_fwd_splitk_elems is positive"""
    from dmayolo._lib import KERN
    want = json.load(open(FIXTURE))['rows']
    seen = {v for w in want for v in w[24:27]}
    assert seen == set(KERN.values()) - {KERN['SPLITK']}, sorted(set(KERN.values()) - seen)
    assert any(w[29] > 0 for w in want) and any(w[29] == 0 for w in want)


if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'dma-yolo_amd'), HERE]
    from dmayolo import _lib
    with open(FIXTURE, 'w') as f:
        f.write('{"columns": "N H W C xps K KH KW S P OH OW yps | offset of a b c (-1 = null) | acc | fp32 then bf16: '
                'route fwd dgrad wgrad, bn_rows, bn_rows with bias, splitk_elems, wgrad_ws_elems",\n "rows": [\n')
        f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in record(_lib.lib)))
        f.write('\n]}\n')
    print(_lib.LIB_PATH, len(rows()), 'rows', os.path.getsize(FIXTURE), 'bytes')
