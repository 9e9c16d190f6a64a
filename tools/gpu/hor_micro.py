"""Micro-benchmark of the depthwise 7x7 kernels of csrc/dwconv.hip (get_dwconv of GnConv, models/common.py:1361-1362) at
the sizes of one C3HB(256) level of a 1536 px image: c_ = 128, so GnConv's depthwise conv runs over sum(dims) = 248
channels of the 192 x 192 stride-8 map.  bf16, each launch captured into a HIP graph of its own and replayed; kernel and
a plain copy of the same algorithmic bytes (dmy_slice_copy over one M x C tensor: one read, one write) alternate, median
of --reps replays after one warm-up.  Every tensor is larger than the 256 MB Infinity Cache.  A report, not a gate.

    python tools/gpu/hor_micro.py [--batch 32] [--reps 7]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dma-yolo_amd')]
from dmayolo.functional import call, prep_weight, ptr, stream  # noqa: E402

CL = torch.channels_last
K, P = 7, 3


def act(n, c, h, w):
    return torch.randn(n, c, h, w, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=CL)


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def timed(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def ab(name, kern, copy, nbytes, reps):
    gk, gc = graphed(kern), graphed(copy)
    timed(gk), timed(gc)
    tk, tc = [], []
    for _ in range(reps):
        tk.append(timed(gk))
        tc.append(timed(gc))
    k, c = sorted(tk)[reps // 2], sorted(tc)[reps // 2]
    print(f'| {name} | {k:.1f} us | {nbytes / 1e9:.2f} GB | {nbytes / k / 1e6:.2f} TB/s | {c:.1f} us | {k / c:.2f}x |', flush=True)


def dw7(N, H, W, C, reps):
    M, es = N * H * W, 2
    x, dz, y = act(N, C, H, W), act(N, C, H, W), act(N, C, H, W)
    w = prep_weight(torch.randn(C, 1, K, K, device='cuda') / K, torch.bfloat16, True)[1]
    b = torch.randn(C, device='cuda')
    rows = call('dmy_dwconv_wgrad_rows', M, C)
    part = torch.empty(rows * (K * K + 1) * C, device='cuda')
    geo = (N, H, W, C, C, K, K, 1, P, H, W, C)
    copy = lambda: call('dmy_slice_copy', 1, ptr(x), C, ptr(y), C, M, C, None, 0, 0, 0.0, 0, stream())  # noqa: E731
    tag = f'{N} x {H}^2 x {C}'
    ab(f'{tag} forward + bias', lambda: call('dmy_dwconv_fwd_act', 1, ptr(x), ptr(w), ptr(b), ptr(y), *geo, None, None, 0,
                                             None, 0, stream()), copy, 2 * M * C * es, reps)
    ab(f'{tag} data-grad', lambda: call('dmy_dwconv_dgrad', 1, ptr(dz), ptr(w), ptr(y), 0, *geo, stream()), copy,
       2 * M * C * es, reps)
    ab(f'{tag} weight-grad + bias-grad', lambda: call('dmy_dwconv_wgrad_bias', 1, ptr(x), ptr(dz), ptr(part), *geo, stream()),
       copy, 2 * M * C * es, reps)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    print('| launch | time | algorithmic bytes | rate | copy of the same bytes | ratio |\n|---|---|---|---|---|---|')
    dw7(a.batch, 192, 192, 248, a.reps)
