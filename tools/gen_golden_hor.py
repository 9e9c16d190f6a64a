"""Capture the reference's get_dwconv(dim, 7, True) (models/common.py:1361-1362, the depthwise conv of GnConv) on its own
PyTorch-CPU path in fp32 (in-container only, like tools/gen_golden_dm.py).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_hor.py
Writes tests/golden/dw7.npz (data only, none of the reference's code): for C0 in (4, 8) -- one 16-byte vector of fp32 /
bf16 -- and the three small shapes of tests/test_gpu_dw7.py, (N, H, W, C) = (2, 5, 6, C0), (1, 7, 9, 3 C0) and
(2, 16, 20, C0), the keys '<C0>.<i>.x / w / b / dz' (inputs) and '.y / dx / dw / db' (the module's output and the
gradients of sum(y * dz)).  The test's fourth shape, (2, 40, 44, 17 C0), is not here: its x and dz alone are 3.8 MB in
fp32 at C0 = 8, over the 1 MiB a committed file may have; the test draws that case from a seeded generator.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the import shim, imports the reference)

C, OUT, npy = G.C, G.OUT, G.npy
SHAPES = [(2, 5, 6, 1), (1, 7, 9, 3), (2, 16, 20, 1)]  # (N, H, W, channel vectors)


def gen_dw7():
    d, gen = {}, torch.Generator().manual_seed(707)
    for c0 in (4, 8):
        for i, (N, H, W, cv) in enumerate(SHAPES):
            ch = cv * c0
            m = C.get_dwconv(ch, 7, True)
            with torch.no_grad():
                m.weight.copy_(torch.randn(ch, 1, 7, 7, generator=gen) / 7)
                m.bias.copy_(torch.randn(ch, generator=gen))
            x = torch.randn(N, ch, H, W, generator=gen).requires_grad_(True)
            dz = torch.randn(N, ch, H, W, generator=gen)
            y = m(x)
            (y * dz).sum().backward()
            for k, v in (('x', x), ('w', m.weight), ('b', m.bias), ('dz', dz), ('y', y), ('dx', x.grad),
                         ('dw', m.weight.grad), ('db', m.bias.grad)):
                d[f'{c0}.{i}.{k}'] = npy(v)
    meta = dict(module='get_dwconv', args=['C', 7, True], shapes=SHAPES, c0=[4, 8])
    np.savez_compressed(os.path.join(OUT, 'dw7.npz'), meta=json.dumps(meta), **d)
    print('wrote dw7', sum(v.nbytes for v in d.values()) / 1e6, 'MB')


if __name__ == '__main__':
    gen_dw7()
