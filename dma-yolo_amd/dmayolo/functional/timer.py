"""KernelTimer: per-launch HIP-event timing of the conv kernels (bench.py's roofline)."""
import torch

from .._lib import call


class KernelTimer:
    """Live per-launch timing of the implicit-GEMM conv kernels with HIP events on the launch
    stream (bench.py roofline).  Off by default; zero overhead when disabled."""
    enabled = False
    records = []  # (kind, algorithmic_flops, algorithmic_bytes, start_event, end_event, shape tag)

    @classmethod
    def run(cls, kind, flops, name, *args, tag=None, nbytes=0.0):
        """nbytes: algorithmic HBM bytes of the launch (operands read once, result written once)"""
        if not cls.enabled:
            return call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(name, *args)
        e1.record()
        cls.records.append((kind, flops, nbytes, e0, e1, tag))

    @classmethod
    def summary(cls, detail=None, peak_flops=2.5e15, peak_bw=8.0e12, peak_flops_f8=5.0e15, table=None):
        """Per-kind totals: launches, flops, seconds, bytes, and the roofline time sum_launches max(F / peak_flops,
        B / peak_bw) split by the binding resource (troof_mfma / troof_hbm).  When `detail` is a dict it also
        receives per-(kind, shape) [launches, flops, seconds, bytes]; when `table` is a list it receives one
        (kind, shape tag, flops, bytes, seconds, roofline seconds) tuple per launch, in launch order."""
        torch.cuda.synchronize()
        out = {}
        for kind, fl, nb, e0, e1, tag in cls.records:
            t = e0.elapsed_time(e1) * 1e-3
            tm, th = fl / (peak_flops_f8 if kind.endswith('_f8') else peak_flops), nb / peak_bw
            if table is not None:
                table.append((kind, tag, fl, nb, t, max(tm, th)))
            d = out.setdefault(kind, [0, 0.0, 0.0, 0.0, 0.0, 0.0])
            d[0] += 1
            d[1] += fl
            d[2] += t
            d[3] += nb
            d[4 if tm >= th else 5] += max(tm, th)
            if detail is not None:
                d = detail.setdefault((kind, tag), [0, 0.0, 0.0, 0.0])
                d[0] += 1
                d[1] += fl
                d[2] += t
                d[3] += nb
        cls.records = []
        return {k: dict(launches=v[0], flops=v[1], seconds=v[2], bytes=v[3], troof_mfma=v[4], troof_hbm=v[5])
                for k, v in out.items()}
