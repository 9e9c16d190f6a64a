"""AutoShape timings: what it costs to get from a decoded host image to the stem input, and from the NMS rows back
to the image (DESIGN.md §3.4 "AutoShape").
python tools/gpu/autoshape_bench.py [out.json]

DMA-YOLO-l bf16, size=1536, batch 1, one 1080 x 1920 and one 3000 x 4000 random uint8 image.  Host clock around work
that ends in a device synchronise; warm-up, then the median of repeated runs.
  * pre-process, host route: data.letterbox + transpose + ascontiguousarray + upload + Model.to_input;
  * pre-process, device route: one pinned non-blocking upload (image, tables, descriptor) + dmy_letterbox_batch;
  * post-process, torch route: scale_coords + xyxy2xywh + the two gn divisions with torch ops on the device rows;
  * post-process, device route: one dmy_scale_boxes launch (geometry upload included);
  * beside them the detect itself: the eager forward + NMS at the letterboxed shape, and the graph-replayed
    detect p50 at 1536 x 1536 from a device tensor.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dma-yolo_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from dmayolo.data import letterbox  # noqa: E402
from dmayolo.infer import GraphedDetector  # noqa: E402
from dmayolo.models.common import autoshape_geometry, letterbox_batch, scale_boxes  # noqa: E402
from dmayolo.synthetic import images  # noqa: E402
from dmayolo.utils.general import non_max_suppression, scale_coords, xyxy2xywh  # noqa: E402

SIZE = 1536


def median_ms(fn, warm, n):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ms)[n // 2], 3)


def main():
    dev = torch.device('cuda', 0)
    m = bench.build(list(bench.CONFIGS['dma-1536']), torch.bfloat16, dev).eval()
    gs = int(m.stride.max())
    rng = np.random.default_rng(0)
    res = {}
    with torch.no_grad():
        for H0, W0 in ((1080, 1920), (3000, 4000)):
            im = rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
            shape1, geo = autoshape_geometry([(H0, W0)], SIZE, gs)
            s2d = bool(m._s2d_stem(torch.empty((1, 3, *shape1), device='meta')))
            stage = [None]

            def host_pre():
                x = letterbox(im, new_shape=shape1, auto=False)[0][None]
                x = np.ascontiguousarray(x.transpose((0, 3, 1, 2)))
                return m.to_input(torch.from_numpy(x).to(dev))

            def dev_pre():
                return letterbox_batch([im], shape1, geo, m.act_dtype, s2d, dev, stage=stage)

            a, b = host_pre(), dev_pre()
            assert torch.equal(a, b), 'the two pre-process routes differ'
            r = res[f'{H0}x{W0}'] = dict(shape1=shape1, s2d=s2d)
            for k in range(2):  # alternate the two routes in one process
                r.setdefault('pre_host_ms', []).append(median_ms(host_pre, 1, 3))
                r.setdefault('pre_device_ms', []).append(median_ms(dev_pre, 5, 30))

            # post-process on 300 kept rows (random boxes on the canvas)
            max_det, keep = 1000, 300
            g = torch.Generator().manual_seed(1)
            rows = (torch.rand((1, max_det, 6), generator=g) * SIZE).to(dev)
            gn = torch.tensor([W0, H0, W0, H0, 1, 1], device=dev)

            def torch_post():
                p = scale_coords(shape1, rows[0, :keep].clone(), (H0, W0))
                wh = xyxy2xywh(p)
                return p, wh, p / gn, wh / gn

            def dev_post():
                return scale_boxes(rows.clone(), [keep], geo, [(H0, W0)])

            for k in range(2):
                r.setdefault('post_torch_ms', []).append(median_ms(torch_post, 10, 50))
                r.setdefault('post_device_ms', []).append(median_ms(dev_post, 10, 50))

            x = dev_pre()
            r['forward_nms_eager_ms'] = median_ms(
                lambda: non_max_suppression(m(x)[0], 0.25, 0.45, max_det=1000), 5, 30)
            print(f'{H0}x{W0}', json.dumps(r), flush=True)

        xs = images(1, SIZE, seed=3, device='cuda')
        gd = GraphedDetector(m)
        res['detect_graph_p50_ms_1536x1536'] = median_ms(lambda: gd.detect(xs, 0.25, 0.45, max_det=1000), 10, 50)
        print(json.dumps({'detect_graph_p50_ms_1536x1536': res['detect_graph_p50_ms_1536x1536']}), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
