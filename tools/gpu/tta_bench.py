"""Test-time augmentation timings (DESIGN.md §3.4 "Test-time augmentation").
python tools/gpu/tta_bench.py [out.json] [--count]   (--count: only the kernel counts, a run of their own)

  * graph-replayed detect p50 (bs1 uint8 -> forward(s) -> NMS 0.25 / 0.45 / max_det 1000, one graph, host clock around
    replay + synchronise), augment=False and augment=True, yolov5s @640 and DMA-YOLO-l @1536; with --count the
    device kernels of one eager call of each instead (torch.profiler), which are the nodes the graph records;
  * at 1536: the five dmy_tta_image launches against the same inputs composed from torch ops (float / 255, flip,
    F.interpolate, F.pad, Model.to_input), and the six dmy_detect_decode_tta launches against Detect.decode + the
    in-place de-scale / de-flip + the clip slices + torch.cat; HIP events, warm-up, median of 30.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dma-yolo_amd')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import bench  # noqa: E402
import dmayolo.functional as Fn  # noqa: E402
from dmayolo.infer import GraphedDetector  # noqa: E402
from dmayolo.synthetic import images  # noqa: E402
from dmayolo.utils.general import non_max_suppression  # noqa: E402


def detect_p50(gd, x, augment, n=60):
    lat = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gd.detect(x, 0.25, 0.45, max_det=1000, augment=augment)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    lat = sorted(lat[10:])
    return round(lat[len(lat) // 2] * 1e3, 3)


def kernel_count(m, x, augment):
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            non_max_suppression(m(x, augment=augment)[0], 0.25, 0.45, max_det=1000)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or 'not measured'
    except Exception as e:  # noqa: BLE001
        return f'not measured ({type(e).__name__})'


def event_median(fn, warm=10, n=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(sorted(ms)[n // 2] * 1e3, 1)  # us


def ends_at_1536(m, x):
    """(fused us, torch us) of the input end and of the output end"""
    import ctypes
    import math
    det = m.model[-1]
    H, W = x.shape[-2:]
    passes, total = m._tta_plan(H, W)
    gs = int(max(m._stride_list()))
    s2d = bool(m._s2d_stem(x))

    def fused_in():
        return [Fn.tta_image(x, m.act_dtype, p[0], p[1], gs, s2d) for p in passes[1:]]

    def torch_in():
        xf = x.float() / 255
        out = []
        for ratio, flip, (oh, ow), (ohp, owp), _, _ in passes[1:]:
            xi = xf.flip(flip) if flip else xf
            if ratio != 1.0:
                xi = F.pad(F.interpolate(xi, size=(oh, ow), mode='bilinear', align_corners=False),
                           [0, owp - ow, 0, ohp - oh], value=0.447)
            out.append(m.to_input(xi))
        return out

    g = torch.Generator().manual_seed(0)
    maps = []
    for _, _, _, (hp, wp), _, _ in passes:
        lv = []
        for ny, nx in m._probe_hw((hp, wp)):
            raw = torch.randn((1, ny, nx, det.na * det.no), generator=g).to(m.act_dtype).cuda()
            lv.append(raw.view(1, ny, nx, det.na, det.no).permute(0, 3, 1, 2, 4))
        maps.append(lv)
    anchors = det.anchors.float().contiguous()
    nl = det.nl
    ls = (ctypes.c_float * nl)(*m._stride_list())

    def fused_out():
        z = torch.empty((1, total, det.no), dtype=torch.float32, device=x.device)
        for (ratio, flip, _, _, mask, zoff), out in zip(passes, maps):
            ys = (ctypes.c_void_p * nl)(*[p.data_ptr() for p in out])
            st = (ctypes.c_long * (3 * nl))(*[v for p in out for v in (p.stride(0), p.stride(2), p.stride(3))])
            hw = (ctypes.c_int * (2 * nl))(*[v for p in out for v in (p.shape[2], p.shape[3])])
            Fn.call('dmy_detect_decode_tta', Fn.dcode(out[0]), nl, ys, st, hw, ls, 1, det.na, det.no, Fn.ptr(anchors),
                    Fn.ptr(z), total, float(ratio), int(flip), float(H), float(W), mask, zoff, Fn.stream())
        return z

    def torch_out():
        y = []
        for (ratio, flip, _, _, _, _), out in zip(passes, maps):
            p = det.decode(out)
            p[..., :4] /= ratio
            if flip == 3:
                p[..., 0] = W - p[..., 0]
            y.append(p)
        gg = sum(4 ** k for k in range(nl))
        y[0] = y[0][:, :-(y[0].shape[1] // gg)]
        y[-1] = y[-1][:, (y[-1].shape[1] // gg) * 4 ** (nl - 1):]
        return torch.cat(y, 1)

    assert math.isclose(float((fused_out() - torch_out()).abs().max()), 0.0, abs_tol=1e-3)
    return dict(tta_image_x5_us=event_median(fused_in), torch_input_x5_us=event_median(torch_in),
                decode_tta_x6_us=event_median(fused_out), torch_output_x6_us=event_median(torch_out))


def main():
    res = {}
    count = '--count' in sys.argv
    argv = [a for a in sys.argv[1:] if a != '--count']
    with torch.no_grad():
        for cfg in ('v5s-640', 'dma-1536'):
            m = bench.build(list(bench.CONFIGS[cfg]), torch.bfloat16, torch.device('cuda', 0)).eval()
            x = images(1, bench.CONFIGS[cfg][2], seed=3, device='cuda')
            gd = GraphedDetector(m)
            r = res[cfg] = {}
            if count:
                for aug in (False, True):
                    m(x, augment=aug)  # warm: the counted call makes no cache-filling launches
                    r[f'kernels_augment_{aug}'] = kernel_count(m, x, aug)
            else:
                for _ in range(2):  # alternate the two forms in one process
                    for aug in (False, True):
                        r.setdefault(f'detect_p50_ms_augment_{aug}', []).append(detect_p50(gd, x, aug))
                if cfg == 'dma-1536':
                    r.update(ends_at_1536(m, x))
            print(cfg, json.dumps(r), flush=True)
            del gd, m
            torch.cuda.empty_cache()
    if argv:
        with open(argv[0], 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
