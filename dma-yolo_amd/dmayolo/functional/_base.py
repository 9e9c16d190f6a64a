"""Tensor and layout helpers every other module of the package builds on: dtype codes, NHWC addressing (pixel
strides), allocation, the output-into-slice rule and the 16-byte vector contract of the streaming kernels.  Imports
nothing from the package."""
import ctypes

import torch


DT = {torch.float32: 0, torch.bfloat16: 1}
CL = torch.channels_last


def dcode(t):
    try:
        return DT[t.dtype]
    except KeyError:
        raise TypeError(f'dmayolo kernels take float32 or bfloat16 activations, got {t.dtype}')


def pixel_stride(t):
    """Return (t', ps) with t' NHWC-addressable: addr(b,c,h,w) = b*H*W*ps + (h*W+w)*ps + c."""
    N, C, H, W = t.shape
    for attempt in range(2):
        s = t.stride()
        if C == 1 or s[1] == 1:
            ps = s[3] if W > 1 else (s[2] if H > 1 else (s[0] if N > 1 else C))
            if (W == 1 or s[3] == ps) and (H == 1 or s[2] == W * ps) and (N == 1 or s[0] == H * W * ps) and ps >= C:
                return t, ps
        t = t.contiguous(memory_format=CL)
    raise AssertionError('layout')


def new_act(N, C, H, W, like):
    return torch.empty((N, C, H, W), dtype=like.dtype, device=like.device, memory_format=CL)


def f32(n, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


_CONST = {}


def const_vec(n, value, dev):
    """a cached fp32 vector of n copies of value on dev, for kernel arguments that are only read (the unit scale /
    zero shift of the activation-only passes): one fill per (n, value, device) instead of two per layer and step"""
    key = (int(n), float(value), str(dev))
    t = _CONST.get(key)
    if t is None:
        t = torch.full((int(n),), float(value), dtype=torch.float32, device=dev)
        # a fill recorded into a HIP graph only runs at replay: cache only what an eager fill has written
        if not torch.cuda.is_current_stream_capturing():
            _CONST[key] = t
    return t


def out_view(o, shape, like):
    """The output-into-slice rule (see concat_buffer): -> (o, its pixel stride) when the view `o` can take a result of
    `shape` in place of a fresh tensor like `like` -- same shape, dtype and device, NHWC-addressable in place -- else
    (None, None).  The Functions take the view as None or [view], so autograd does not see the buffer as an input."""
    if o is None or tuple(o.shape) != tuple(shape) or o.dtype != like.dtype or o.device != like.device:
        return None, None
    t, ps = pixel_stride(o)  # a view that is not addressable in place comes back as a copy: a fresh output instead
    return (o, ps) if t is o else (None, None)


def out_or_new(out, shape, like):
    """-> (tensor, its pixel stride) for a Function's `out` argument (None or [view]): the view when out_view takes it,
    else a fresh dense activation of `shape`"""
    y, yps = out_view(out and out[0], shape, like)
    if y is None:
        y, yps = new_act(*shape, like), shape[1]
    return y, yps


def concat_buffer(N, Ct, H, W, like):
    """the channels_last buffer of a plain Concat whose producers write their outputs straight into its channel
    slices (conv_bn_act(out=buf[:, c0:c1])); ConcatFn then recognises the in-place slices and copies nothing"""
    return new_act(N, Ct, H, W, like)


VW = {torch.float32: 4, torch.bfloat16: 8}


def vec_ok(dtype, chans=(), strides=(), tensors=()):
    """The 16-byte vector contract of the streaming kernels (csrc/launch.h vec_ok): channel counts and pixel strides in
    multiples of 8 (bf16) / 4 (fp32), 16-byte aligned bases.  False: the caller falls back (vec_view) or refuses."""
    vw = VW[dtype]
    return not (any(c % vw for c in chans) or any(s % vw for s in strides) or any(t.data_ptr() % 16 for t in tensors))


def vec_check(what, dtype, chans=(), strides=(), tensors=(), max_vecs=None):
    """vec_ok for a kernel with no scalar path: NotImplementedError where it fails (or a pixel has over max_vecs vectors)"""
    if not vec_ok(dtype, chans, strides, tensors) or (max_vecs and any(c // VW[dtype] > max_vecs for c in chans)):
        raise NotImplementedError(f'{what}: channel counts {list(chans)} / pixel strides {list(strides)} must be '
                                  f'multiples of {VW[dtype]} for {dtype} and every tensor 16-byte aligned'
                                  + (f', at most {max_vecs} vectors per pixel' if max_vecs else ''))


def vec_view(t):
    """(t', ps) as pixel_stride, copied dense when the view is not 16-byte-vector addressable (an odd slice offset)"""
    t, ps = pixel_stride(t)
    if not vec_ok(t.dtype, (), [ps], [t]):
        t, ps = pixel_stride(t.contiguous(memory_format=CL))
    return t, ps


def vec_pad(C, dtype):
    """C rounded up to a whole number of 16-byte vectors of dtype"""
    return -(-C // VW[dtype]) * VW[dtype]


def zero_padded_channels(x):
    """Channel count the storage of `x` is zero-padded to (set by ToNHWC for the 3-channel stem)."""
    cp = getattr(x, '_dmy_cpad', 0)
    return cp if cp and cp % VW[x.dtype] == 0 else 0


def conv_out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def even_hw(H, W, what):
    """SM folds 2 x 2 pixels into channels: an odd map has no SM layout (the reference's cat fails on it too)"""
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f'{what} needs a map with even height and width (SM folds 2 x 2 pixels into channels, '
                         f'models/common.py:1467), got {H}x{W}')


def ctypes_off(t, c0):
    return ctypes.c_void_p(t.data_ptr() + c0 * t.element_size())
