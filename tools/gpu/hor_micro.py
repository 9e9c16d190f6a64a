"""Micro-benchmark of the depthwise 7x7 kernels of csrc/dwconv.hip (get_dwconv of GnConv, models/common.py:1361-1362) at
the sizes of one C3HB(256) level of a 1536 px image: c_ = 128, so GnConv's depthwise conv runs over sum(dims) = 248
channels of the 192 x 192 stride-8 map.  bf16, each launch captured into a HIP graph of its own and replayed; kernel and
a plain copy of the same algorithmic bytes (dmy_slice_copy over one M x C tensor: one read, one write) alternate, median
of --reps replays after one warm-up.  Every tensor is larger than the 256 MB Infinity Cache.  A report, not a gate.

`--what hor`: the gate and layer-scale kernels of csrc/hor.hip the same way, on the slices GnConv(128) hands them (pwa
of the 256-wide fused_x, dw_list[i] of the 248-wide dw_abc, dense pws outputs), each next to a dense copy that moves the
same number of bytes.  `--what block`: one HorBlock(128) forward + backward at the same map, bf16, an event ahead of
every launch (the launch observer of dmayolo._lib), summed per launch family (the 1x1 convs told apart by their channel
counts); eager, so the host's launch gaps are in the step time.

    python tools/gpu/hor_micro.py [--what dw7 hor block] [--batch 32] [--reps 7]
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


def hor(N, H, W, c, reps):
    M, es, dims = N * H * W, 2, [c // 16, c // 8, c // 4, c // 2, c]
    fused, dw, dfused, ddw = act(N, 2 * c, H, W), act(N, sum(dims), H, W), act(N, 2 * c, H, W), act(N, sum(dims), H, W)
    src, dst = act(N, 5 * c // 2, H, W), act(N, 5 * c // 2, H, W)

    def copy(passes, C):  # `passes` tensors of M x C elements cross the memory bus: a dense copy of half as many
        rows, wide = M * passes * C // 2 // c, c
        return lambda: call('dmy_slice_copy', 1, ptr(src), wide, ptr(dst), wide, rows, wide, None, 0, 0, 0.0, 0, stream())
    off = 0
    for i, d in enumerate(dims):
        a, aps = (fused[:, :d], 2 * c) if i == 0 else (act(N, d, H, W), d)
        da, daps = (dfused[:, :d], 2 * c) if i == 0 else (act(N, d, H, W), d)
        b, db, y, dy = dw[:, off:off + d], ddw[:, off:off + d], act(N, d, H, W), act(N, d, H, W)
        off += d
        ab(f'gate {i} forward, C = {d}', lambda: call('dmy_gate_fwd', 1, ptr(a), aps, ptr(b), sum(dims), ptr(y), d, M, d,
                                                       1.0, stream()), copy(3, d), 3 * M * d * es, reps)
        ab(f'gate {i} backward, C = {d}', lambda: call('dmy_gate_bwd', 1, ptr(dy), d, ptr(a), aps, ptr(b), sum(dims),
                                                        ptr(da), daps, ptr(db), sum(dims), M, d, 1.0, stream()),
           copy(5, d), 5 * M * d * es, reps)
    x, y, o, dy, g = act(N, c, H, W), act(N, c, H, W), act(N, c, H, W), act(N, c, H, W), torch.rand(c, device='cuda') + 0.5
    rows = call('dmy_layerscale_bwd_rows', M)
    part, dg = torch.empty(rows * c, device='cuda'), torch.empty(c, device='cuda')
    ab(f'layer scale forward, C = {c}', lambda: call('dmy_layerscale_fwd', 1, ptr(x), c, ptr(y), ptr(g), ptr(o), c, M, c,
                                                     stream()), copy(3, c), 3 * M * c * es, reps)

    def ls_bwd():
        call('dmy_layerscale_bwd', 1, ptr(x), c, ptr(y), ptr(g), ptr(dy), M, c, ptr(part), stream())
        call('dmy_reduce_rows', ptr(part), rows, c, ptr(dg), 0, stream())
    ab(f'layer scale backward + row sum, C = {c}', ls_bwd, copy(3, c), 3 * M * c * es, reps)


def family(name, args, c):
    ints = {a for a in args if isinstance(a, int)}
    if name.startswith('dmy_dwconv'):
        return 'dw7'
    if name.startswith('dmy_gate'):
        return 'gates'
    if name.startswith('dmy_layerscale'):
        return 'layer scale'
    if name.startswith('dmy_layernorm'):
        return 'LayerNorm'
    if name.startswith(('dmy_conv', 'dmy_bn', 'dmy_reduce_rows', 'dmy_colsum')):
        if 4 * c in ints:
            return 'MLP'
        if 2 * c in ints:
            return 'proj_in'
        if ints & {c // 16, c // 8, c // 4, c // 2}:
            return 'pws'
        return 'proj_out / row sums'
    return 'other: ' + name


def block(N, H, W, c, reps):
    import dmayolo.functional as Fn
    from dmayolo.models.common import HorBlock
    m = HorBlock(c).cuda().train()
    with torch.no_grad():
        m.gamma1.fill_(1.0), m.gamma2.fill_(1.0)
    x = act(N, c, H, W).requires_grad_(True)
    ev = []

    def mark(name, args):  # _lib.call's observer: one event ahead of every launch, from whichever module
        if name.endswith(('_rows', '_blocks', '_ok', '_elems', '_bytes', '_route', '_groups')):
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append((family(name, args, c), e))
    tot = {}
    for it in range(reps + 1):
        ev.clear()
        Fn._lib.TRACE[0] = mark
        try:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            m(x).float().sum().backward()
            t1.record()
            torch.cuda.synchronize()
        finally:
            Fn._lib.TRACE[0] = None
        if it:  # the first pass warms up
            tot.setdefault('whole step (eager, with gaps)', []).append(t0.elapsed_time(t1) * 1e3)
            fam = {}
            # a launch runs from its own event to the next launch's (the last one: to the step's closing event); torch
            # work between two launches (the loss sum, autograd's adds) is counted with the launch ahead of it
            for (f, e0), (_, e1) in zip(ev, ev[1:] + [(None, t1)]):
                fam[f] = fam.get(f, 0.0) + e0.elapsed_time(e1) * 1e3
            for f, v in fam.items():
                tot.setdefault(f, []).append(v)
        m.zero_grad(set_to_none=True)
        x.grad = None
    print(f'\nHorBlock({c}) forward + backward, {N} x {H}^2, bf16, median of {reps}:\n| family | time |\n|---|---|')
    for f, v in sorted(tot.items(), key=lambda kv: -sorted(kv[1])[len(kv[1]) // 2]):
        print(f'| {f} | {sorted(v)[len(v) // 2]:.0f} us |', flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', nargs='+', default=['dw7'], choices=['dw7', 'hor', 'block'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    print('| launch | time | algorithmic bytes | rate | copy of the same bytes | ratio |\n|---|---|---|---|---|---|')
    if 'dw7' in a.what:
        dw7(a.batch, 192, 192, 248, a.reps)
    if 'hor' in a.what:
        hor(a.batch, 192, 192, 128, a.reps)
    if 'block' in a.what:
        block(a.batch, 192, 192, 128, a.reps)
