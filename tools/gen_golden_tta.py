"""Capture the reference's test-time-augmented eval output (models/yolo.py:194-275, augment=True) for the
model_v5s fixture, on its own PyTorch-CPU path in fp32 (in-container only, like tools/gen_golden.py).

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_tta.py
Reads tests/golden/model_v5s.npz (meta.yaml, the sd.* weights, in.0 [2, 3, 64, 64]) and writes
tests/golden/tta_v5s.npz holding only `out` [2, 1308, 15] fp32: data, none of the reference's code.
"""
import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_stubs  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
Y = ref_stubs.install()

torch.set_num_threads(8)


def main():
    z = np.load(os.path.join(GOLDEN, 'model_v5s.npz'), allow_pickle=False)
    meta = json.loads(str(z['meta']))
    model = Y.Model(deepcopy(meta['yaml']), nc=meta['nc'])
    own = model.state_dict()
    sd = {k[3:]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith('sd.')}
    sd = {k: v.to(own[k].dtype) for k, v in sd.items() if k in own}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if not k.endswith('num_batches_tracked')], (missing, unexpected)
    x = torch.from_numpy(np.array(z['in.0'])).float()
    model.eval()
    with torch.no_grad():
        out, none = model(x, augment=True)
    assert none is None and out.dtype == torch.float32 and tuple(out.shape) == (2, 1308, 15), out.shape
    path = os.path.join(GOLDEN, 'tta_v5s.npz')
    np.savez_compressed(path, out=out.numpy().copy())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
