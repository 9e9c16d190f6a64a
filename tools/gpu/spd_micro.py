"""Micro-benchmark of csrc/spd.hip: each fused pass against the launches it replaces, at DM.yaml's layer-1 and
layer-3 shapes of a 1536 px image (the pre-BN map of the 3x3 conv: 768^2 x 128 and 384^2 x 256) and, for DMMConv2's
front end, CADMM2.yaml's inputs there (768^2 x 64 and 384^2 x 384).  bf16, device events, fused and composed launches
alternating, median of --reps after one warm-up; every tensor is far larger than the 256 MB Infinity Cache.

    python tools/gpu/spd_micro.py [--batch 8] [--reps 7]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dma-yolo_amd')]
from dmayolo.functional import call, ptr, stream  # noqa: E402

CL = torch.channels_last


def act(n, c, h, w):
    return torch.randn(n, c, h, w, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=CL)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def ab(name, fused, composed, bytes_f, bytes_c, reps):
    fused(), composed()
    tf, tc = [], []
    for _ in range(reps):
        tf.append(timed(fused))
        tc.append(timed(composed))
    f, c = sorted(tf)[reps // 2], sorted(tc)[reps // 2]
    print(f'| {name} | {f:.1f} us | {bytes_f / 1e9:.2f} GB | {bytes_f / f / 1e6:.2f} TB/s | {c:.1f} us ({bytes_c / 1e9:.2f} GB) '
          f'| {c / f:.2f}x |', flush=True)


def bn_passes(N, H, W, K, reps):
    M, es = N * H * W, 2
    z, dy, t, dz = act(N, K, H, W), act(N, 4 * K, H // 2, W // 2), act(N, K, H, W), act(N, K, H, W)
    y = torch.empty_like(dy)
    v = [torch.rand(K, device='cuda') + 0.5 for _ in range(7)]
    st, co = v[:4], v[4:]
    tag = f'{H}^2 x {K}'
    ab(f'{tag} act forward', lambda: call('dmy_bn_act_s2d_fwd', 1, ptr(z), K, ptr(st[0]), ptr(st[1]), 1, ptr(y), 4 * K, N, H,
                                          W, K, stream()),
       lambda: (call('dmy_bn_act_fwd', 1, ptr(z), K, ptr(st[0]), ptr(st[1]), 1, None, 0, ptr(t), K, M, K, stream()),
                call('dmy_space_to_depth', 1, ptr(t), K, ptr(y), 4 * K, N, H, W, K, 0, stream())),
       2 * M * K * es, 4 * M * K * es, reps)
    P = call('dmy_bn_bwd_reduce_s2d_rows', 1, M, K)
    pa, pb = torch.empty(P * K, device='cuda'), torch.empty(P * K, device='cuda')
    ab(f'{tag} backward reduce', lambda: call('dmy_bn_bwd_reduce_s2d', 1, ptr(z), K, ptr(dy), 4 * K, *map(ptr, st), 1, N, H, W,
                                              K, ptr(pa), ptr(pb), stream()),
       lambda: (call('dmy_space_to_depth', 1, ptr(t), K, ptr(dy), 4 * K, N, H, W, K, 1, stream()),
                call('dmy_bn_bwd_reduce', 1, ptr(z), K, ptr(t), K, *map(ptr, st), 1, M, K, ptr(pa), ptr(pb), stream())),
       2 * M * K * es, 4 * M * K * es, reps)
    ab(f'{tag} backward apply', lambda: call('dmy_bn_bwd_apply_s2d', 1, ptr(z), K, ptr(dy), 4 * K, *map(ptr, st), 1,
                                             *map(ptr, co), ptr(dz), K, N, H, W, K, stream()),
       lambda: (call('dmy_space_to_depth', 1, ptr(t), K, ptr(dy), 4 * K, N, H, W, K, 1, stream()),
                call('dmy_bn_bwd_apply', 1, ptr(z), K, ptr(t), K, *map(ptr, st), 1, *map(ptr, co), ptr(dz), K, M, K,
                     stream())),
       3 * M * K * es, 5 * M * K * es, reps)


def split(N, H, W, C, reps):
    M, es = N * H * W, 2
    x, sm, mp = act(N, C, H, W), act(N, 4 * C, H // 2, W // 2), act(N, C, H // 2, W // 2)
    dx = torch.empty_like(x)
    arg = torch.empty(N * (H // 2) * (W // 2) * C, dtype=torch.uint8, device='cuda')
    pool = M * C // 4 * (es + 1)  # pooled map + argmax
    tag = f'{H}^2 x {C}'
    ab(f'{tag} split forward', lambda: call('dmy_spd_split_fwd', 1, ptr(x), C, ptr(sm), 4 * C, ptr(mp), C, ptr(arg), N, H, W, C,
                                            stream()),
       lambda: (call('dmy_space_to_depth', 1, ptr(x), C, ptr(sm), 4 * C, N, H, W, C, 0, stream()),
                call('dmy_maxpool2_fwd', 1, ptr(x), C, ptr(mp), C, ptr(arg), N, H, W, C, stream())),
       2 * M * C * es + pool, 3 * M * C * es + pool, reps)
    ab(f'{tag} split backward', lambda: call('dmy_spd_split_bwd', 1, ptr(sm), 4 * C, ptr(mp), C, ptr(arg), ptr(dx), C, N, H, W,
                                             C, stream()),
       lambda: (call('dmy_space_to_depth', 1, ptr(dx), C, ptr(sm), 4 * C, N, H, W, C, 1, stream()),
                call('dmy_maxpool2_bwd', 1, ptr(mp), C, ptr(arg), ptr(dx), C, 1, N, H, W, C, stream())),
       2 * M * C * es + pool, 4 * M * C * es + pool, reps)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    print('| pass | fused | bytes | rate | launches it replaces (bytes) | ratio |\n|---|---|---|---|---|---|')
    bn_passes(a.batch, 768, 768, 128, a.reps)
    bn_passes(a.batch, 384, 384, 256, a.reps)
    split(a.batch, 768, 768, 64, a.reps)
    split(a.batch, 384, 384, 384, a.reps)
