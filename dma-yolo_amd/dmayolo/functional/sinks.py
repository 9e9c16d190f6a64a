"""Gradient sinks: where a backward kernel writes the gradient of an input that has several consumers.

The protocol is duck-typed.  A sink (GradSink, or one channel slice of a SliceSink: _SlicePart) offers

    target(N, C, H, W, like) -> (buffer, pixel stride, accumulate flag): where the kernel writes, and whether it adds
    peek(N, C, H, W)         -> (buffer, pixel stride) that target() would return now, or None when it would allocate
    done()                   -> what the backward returns for that input after the launch: the finished buffer from the
                                last contributor, None from the others (a _SlicePart: its slice view)
    passthrough(g)           -> the same for an identity contribution (residual, concat slice): g is adopted or added in

and a backward never calls them directly: sink_target / sink_result wrap target / done for a sink that may be None (a
fresh buffer, returned as it is), pass_or_self wraps passthrough, and _write_target serves a kernel that cannot
accumulate.  A Function takes its sinks as plain forward arguments and keeps them on ctx."""
import torch

from .._lib import call, ptr, stream
from ._base import CL, dcode, new_act, pixel_stride


class GradSink:
    """Input-gradient accumulator for an activation with several consumers inside one module.

    Autograd would sum the consumers' gradient contributions with separate add kernels.  Here
    the consumers' backward kernels write (first contribution in backward order) or accumulate
    (the rest, through the kernels' accumulate flags) into one NHWC buffer, and only the LAST of
    the `n` contributions hands the finished buffer to autograd (the others return None).  The
    activation's producer runs only after all of its consumers' backwards, and any contribution
    from outside the module is added by autograd to the finished buffer.  The sink resets after
    the n-th contribution, so a retained graph can run backward again.  adopt=False: a first passthrough contribution
    is copied into a fresh buffer instead of becoming the buffer, for a gradient that later contributions must not
    accumulate into (GhostConv: the slice of an upstream gradient that other branches still read).
    """
    __slots__ = ('n', 'seen', 'buf', 'ps', 'adopt')

    def __init__(self, n, adopt=True):
        self.n, self.seen, self.buf, self.ps, self.adopt = n, 0, None, 0, adopt

    def expect(self, k):
        """register k more contributions (a consumer module taking this sink from its caller, in forward)"""
        self.n += k
        return self

    def _tick(self):
        self.seen += 1
        if self.seen < self.n:
            return None
        ret = self.buf
        self.buf, self.seen = None, 0
        return ret

    def target(self, N, C, H, W, like):
        """-> (buffer, pixel stride, accumulate flag, tensor to hand to autograd or None); call
        `done()` after the kernel has been launched"""
        if self.buf is None:
            self.buf, self.ps = new_act(N, C, H, W, like), C
            return self.buf, C, 0
        return self.buf, self.ps, 1

    def peek(self, N, C, H, W):
        """(buffer, pixel stride) a target() call would return now without allocating, or None when it would
        allocate a fresh dense buffer"""
        return (self.buf, self.ps) if self.buf is not None else None

    def done(self):
        return self._tick()

    def passthrough(self, g):
        """identity contribution (a residual / concat slice): adopt g as the buffer, or add it in.
        Adoption is safe for the residual pattern: every other reader of g lies inside the branch,
        whose backwards all finish before the branch's first consumer accumulates into g."""
        g, gps = pixel_stride(g)
        if self.buf is None and self.adopt:
            self.buf, self.ps = g, gps
        else:
            N, C, H, W = g.shape
            acc = int(self.buf is not None)
            if not acc:
                self.buf, self.ps = new_act(N, C, H, W, g), C
            call('dmy_slice_copy', dcode(g), ptr(g), gps, ptr(self.buf), self.ps, N * H * W, C, None, 0, 0, 0.0, acc,
                 stream())
        return self._tick()


def sink_target(sink, N, C, H, W, like):
    """-> (buffer, pixel stride, accumulate flag) for an input gradient; see sink_result"""
    if sink is None:
        return new_act(N, C, H, W, like), C, 0
    return sink.target(N, C, H, W, like)


def sink_result(sink, buf):
    """what the backward returns for that input: its own buffer, or the sink's verdict"""
    return buf if sink is None else sink.done()


def pass_or_self(sink, g):
    """what the backward returns for an input whose gradient is g itself (a residual, a concat slice)"""
    return g if sink is None else sink.passthrough(g)


class SliceSink:
    """Gradient buffer of an activation that is only read through channel slices (torch.split, models/common.py:1347,
    1351).  The consumers' backward kernels write their slice's gradient straight into this one NHWC buffer through
    `part(c0, C)`, which follows the GradSink protocol (target / peek / done / passthrough), and the n-th SplitFn
    backward hands the finished buffer to autograd (the others return None): no zero-filled slice gradients, no adds.
    The slices must cover every channel.  Resets after the n-th contribution, like GradSink."""
    __slots__ = ('n', 'seen', 'buf', 'shape', 'dtype', 'device')

    def __init__(self, n, like):
        self.n, self.seen, self.buf = n, 0, None
        self.shape, self.dtype, self.device = tuple(like.shape), like.dtype, like.device

    def view(self, c0, C):
        if self.buf is None:
            self.buf = torch.empty(self.shape, dtype=self.dtype, device=self.device, memory_format=CL)
        return self.buf[:, c0:c0 + C]

    def part(self, c0, C):
        return _SlicePart(self, c0, C)

    def tick(self):
        self.seen += 1
        if self.seen < self.n:
            return None
        ret = self.buf
        self.buf, self.seen = None, 0
        return ret


class _SlicePart:
    """one channel slice of a SliceSink as a kernel's gradient target: always written, never accumulated; the slice
    view is what the backward returns, and SplitFn.backward recognises it as already in place"""
    __slots__ = ('sink', 'c0', 'C')

    def __init__(self, sink, c0, C):
        self.sink, self.c0, self.C = sink, c0, C

    def target(self, N, C, H, W, like):
        return self.sink.view(self.c0, self.C), self.sink.shape[1], 0

    def peek(self, N, C, H, W):
        return self.sink.view(self.c0, self.C), self.sink.shape[1]

    def done(self):
        return self.sink.view(self.c0, self.C)

    def passthrough(self, g):
        g, gps = pixel_stride(g)
        v = self.sink.view(self.c0, self.C)
        N, C, H, W = g.shape
        call('dmy_slice_copy', dcode(g), ptr(g), gps, ptr(v), self.sink.shape[1], N * H * W, C, None, 0, 0, 0.0, 0,
             stream())
        return v


class SplitFn(torch.autograd.Function):
    """x[:, c0:c0 + C] as a view (one output of torch.split); the gradient goes into `sink` (a SliceSink over x's
    channels, or None: a zero-filled gradient with the slice copied in)."""

    @staticmethod
    def forward(ctx, x, c0, C, sink=None):
        ctx.c0, ctx.C, ctx.sink, ctx.xshape = c0, C, sink, tuple(x.shape)
        return x[:, c0:c0 + C]

    @staticmethod
    def backward(ctx, g):
        sink = ctx.sink
        if sink is None:
            sink = SliceSink(1, torch.empty(ctx.xshape, dtype=g.dtype, device='meta'))
            sink.device = g.device
            sink.view(0, ctx.xshape[1]).zero_()
        v = sink.view(ctx.c0, ctx.C)
        if g.data_ptr() != v.data_ptr() or g.stride() != v.stride() or g.dtype != v.dtype:
            _SlicePart(sink, ctx.c0, ctx.C).passthrough(g.to(v.dtype))
        return sink.tick(), None, None, None


def _write_target(sink, N, C, H, W, like):
    """-> (buffer, pixel stride, finish) for a backward kernel that writes but cannot accumulate: the sink's buffer
    when this is its first contribution (or a SliceSink part), else a fresh tensor that finish() adds into the sink"""
    buf, ps, acc = sink_target(sink, N, C, H, W, like)
    if not acc:
        return buf, ps, lambda: sink_result(sink, buf)
    tmp = new_act(N, C, H, W, like)
    return tmp, C, lambda: sink.passthrough(tmp)
