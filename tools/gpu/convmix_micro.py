"""Micro-benchmark of the depthwise 9x9 kernels of csrc/dwconv.hip and the act-then-BN passes of csrc/convmix.hip (ConvMix,
models/cspcm.py:25-41), bf16, at two tensors: the inner map of CSPCM.yaml's layer 12 at 1536 px (c_ = 2048 channels of
the 48 x 48 stride-32 map) and tools/gpu/hor_micro.py's 248-channel 192 x 192 map, where the 7x7 launches run in the same
process.  Each launch is captured into a HIP graph of its own and replayed; kernel and a plain copy of the same
algorithmic bytes (dmy_slice_copy: one read, one write, over as many rows as move that many bytes) alternate, median of
--reps replays after one warm-up.  Every tensor is larger than the 256 MB Infinity Cache.  The act-BN passes are timed
next to dmy_bn_act_fwd / dmy_bn_bwd_reduce / dmy_bn_bwd_apply on the same tensors (up to 2048 bf16 channels, the widest
the bn.hip vector kernels take).  A report, not a gate.

    python tools/gpu/convmix_micro.py [--batch 32] [--reps 7] [--what dw actbn] [--ks 3 5 --stride 2]

--ks times the depthwise launches of those filter sizes (3 / 5 / 7 / 9) at --stride instead of the default 9x9 / 7x7 sets.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dma-yolo_amd'), os.path.dirname(os.path.abspath(__file__))]
from dmayolo.functional import call, prep_weight, ptr, stream  # noqa: E402
from hor_micro import act, graphed, timed  # noqa: E402

GELU, SILU = 4, 1
RESULTS = {}


def ab(name, kern, copy, nbytes, reps):
    gk, gc = graphed(kern), graphed(copy)
    timed(gk), timed(gc)
    tk, tc = [], []
    for _ in range(reps):
        tk.append(timed(gk))
        tc.append(timed(gc))
    k, c = sorted(tk)[reps // 2], sorted(tc)[reps // 2]
    RESULTS[name] = k
    print(f'| {name} | {k:.1f} us | {nbytes / 1e9:.2f} GB | {nbytes / k / 1e6:.2f} TB/s | {c:.1f} us | {k / c:.2f}x |', flush=True)


def copier(src, dst, M, C, tensors):
    """a dense copy that moves `tensors` M x C tensors' worth of bytes (one read + one write of tensors / 2 of them)"""
    rows = M * tensors // 2
    assert rows * C <= src.numel() and rows * C <= dst.numel()
    return lambda: call('dmy_slice_copy', 1, ptr(src), C, ptr(dst), C, rows, C, None, 0, 0, 0.0, 0, stream())


def dw(N, H, W, C, reps, ks, S=1):
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1  # padding k // 2, k odd
    M, es = N * OH * OW, 2
    x, dz, y = act(N, C, H, W), act(N, C, OH, OW), act(N, C, H, W)
    b = torch.randn(C, device='cuda')
    tag = f'{N} x {H}^2 x {C}' + (f' s{S}' if S != 1 else '')
    copy = copier(x, y, M, C, 2)
    for K in ks:
        P = K // 2
        w = prep_weight(torch.randn(C, 1, K, K, device='cuda') / K, torch.bfloat16, True)[1]
        rows, frows = call('dmy_dwconv_wgrad_rows', M, C), call('dmy_dwconv_fwd_rows', M, C)
        part = torch.empty(rows * K * K * C, device='cuda')
        ps, pq = torch.empty(frows * C, device='cuda'), torch.empty(frows * C, device='cuda')
        geo = (N, H, W, C, C, K, K, S, P, OH, OW, C)
        ab(f'{tag} {K}x{K} forward + BN partial rows', lambda: call('dmy_dwconv_fwd', 1, ptr(x), ptr(w), ptr(b), ptr(y), ptr(ps),
                                                                   ptr(pq), *geo, stream()), copy, 2 * M * C * es, reps)
        if K == 9:
            sc, sh = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
            ab(f'{tag} 9x9 inference forward (fwd_actbn, GELU, residual)',
               lambda: call('dmy_dwconv_fwd_actbn', 1, ptr(x), ptr(w), ptr(b), ptr(y), *geo, ptr(sc), ptr(sh), GELU, ptr(x),
                            C, stream()), copy, 2 * M * C * es, reps)
        ab(f'{tag} {K}x{K} data-grad', lambda: call('dmy_dwconv_dgrad', 1, ptr(dz), ptr(w), ptr(y), 0, *geo, stream()), copy,
           2 * M * C * es, reps)
        ab(f'{tag} {K}x{K} weight-grad (partial rows)', lambda: call('dmy_dwconv_wgrad', 1, ptr(x), ptr(dz), ptr(part), *geo,
                                                                    stream()), copy, 2 * M * C * es, reps)
        del part
    if sorted(ks) == [7, 9]:
        print(f'\n{tag}: time per tap, 9x9 (us / 81) against 7x7 (us / 49)')
        for what in ('forward + BN partial rows', 'data-grad', 'weight-grad (partial rows)'):
            t9, t7 = RESULTS[f'{tag} 9x9 {what}'] / 81, RESULTS[f'{tag} 7x7 {what}'] / 49
            print(f'| {what} | {t9:.2f} us / tap | {t7:.2f} us / tap | {t9 / t7:.2f}x |', flush=True)
        print()


def actbn(N, H, W, C, reps):
    M, es = N * H * W, 2
    z, dy, y = act(N, C, H, W), act(N, C, H, W), act(N, C, H, W)
    z.mul_(1.5)
    tag = f'{N} x {H}^2 x {C}'
    P = call('dmy_bn_partial_rows', M)
    R = call('dmy_bn_reduce_rows', 1, ptr(z), C, ptr(dy), C, M, C)
    pa, pb = torch.empty(max(P, R) * C, device='cuda'), torch.empty(max(P, R) * C, device='cuda')
    cs, cd = (torch.empty(3 * M // 2 * C, device='cuda', dtype=torch.bfloat16) for _ in range(2))  # the copies' own buffers
    sc, sh = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda') * 0.1
    mean, invstd = torch.randn(C, device='cuda') * 0.1, torch.rand(C, device='cuda') + 0.5
    ca, cb, cc = sc.clone(), torch.randn(C, device='cuda') * 0.01, torch.randn(C, device='cuda') * 0.01
    ab(f'{tag} actbn_stats', lambda: call('dmy_actbn_stats', 1, ptr(z), C, GELU, M, C, ptr(pa), ptr(pb), stream()),
       copier(cs, cd, M, C, 1), M * C * es, reps)
    ab(f'{tag} bn_stats (no activation)', lambda: call('dmy_bn_stats', 1, ptr(z), C, M, C, ptr(pa), ptr(pb), stream()),
       copier(cs, cd, M, C, 1), M * C * es, reps)
    ab(f'{tag} actbn_fwd (GELU)', lambda: call('dmy_actbn_fwd', 1, ptr(z), C, GELU, ptr(sc), ptr(sh), None, 0, ptr(y), C, M,
                                                 C, stream()), copier(cs, cd, M, C, 2), 2 * M * C * es, reps)
    ab(f'{tag} bn_act_fwd (GELU)', lambda: call('dmy_bn_act_fwd', 1, ptr(z), C, ptr(sc), ptr(sh), GELU, None, 0, ptr(y), C,
                                                  M, C, stream()), copier(cs, cd, M, C, 2), 2 * M * C * es, reps)
    ab(f'{tag} bn_act_fwd (SiLU)', lambda: call('dmy_bn_act_fwd', 1, ptr(z), C, ptr(sc), ptr(sh), SILU, None, 0, ptr(y), C,
                                                  M, C, stream()), copier(cs, cd, M, C, 2), 2 * M * C * es, reps)
    ab(f'{tag} actbn_bwd_reduce', lambda: call('dmy_actbn_bwd_reduce', 1, ptr(z), C, ptr(dy), C, ptr(mean), ptr(invstd),
                                                GELU, M, C, ptr(pa), ptr(pb), stream()), copier(cs, cd, M, C, 2),
       2 * M * C * es, reps)
    ab(f'{tag} bn_bwd_reduce (GELU)', lambda: call('dmy_bn_bwd_reduce', 1, ptr(z), C, ptr(dy), C, ptr(sc), ptr(sh), ptr(mean),
                                                     ptr(invstd), GELU, M, C, ptr(pa), ptr(pb), stream()),
       copier(cs, cd, M, C, 2), 2 * M * C * es, reps)
    ab(f'{tag} actbn_bwd_apply + bias rows', lambda: call('dmy_actbn_bwd_apply', 1, ptr(z), C, ptr(dy), C, ptr(mean),
                                                           ptr(invstd), GELU, ptr(ca), ptr(cb), ptr(cc), ptr(y), C, M, C,
                                                           ptr(pa), stream()), copier(cs, cd, M, C, 3), 3 * M * C * es, reps)
    ab(f'{tag} bn_bwd_apply (GELU)', lambda: call('dmy_bn_bwd_apply', 1, ptr(z), C, ptr(dy), C, ptr(sc), ptr(sh), ptr(mean),
                                                    ptr(invstd), GELU, ptr(ca), ptr(cb), ptr(cc), ptr(y), C, M, C, stream()),
       copier(cs, cd, M, C, 3), 3 * M * C * es, reps)
    ab(f'{tag} bn_bwd_apply (SiLU)', lambda: call('dmy_bn_bwd_apply', 1, ptr(z), C, ptr(dy), C, ptr(sc), ptr(sh), ptr(mean),
                                                    ptr(invstd), SILU, ptr(ca), ptr(cb), ptr(cc), ptr(y), C, M, C, stream()),
       copier(cs, cd, M, C, 3), 3 * M * C * es, reps)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', nargs='+', default=['dw', 'actbn'], choices=['dw', 'actbn'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ks', type=int, nargs='+', choices=[3, 5, 7, 9], help='time these depthwise filter sizes only')
    ap.add_argument('--stride', type=int, default=1, choices=[1, 2], help='with --ks (7 and 9 are stride 1 only)')
    a = ap.parse_args()
    print('| launch | time | algorithmic bytes | rate | copy of the same bytes | ratio |\n|---|---|---|---|---|---|')
    for (H, C, ks) in ((48, 2048, (9,)), (192, 248, (9, 7))):
        if 'dw' in a.what:
            dw(a.batch, H, H, C, a.reps, a.ks or ks, a.stride if a.ks else 1)
        if 'actbn' in a.what:
            actbn(a.batch, H, H, C, a.reps)
