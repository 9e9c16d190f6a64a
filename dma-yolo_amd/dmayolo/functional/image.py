"""Image -> stem input (csrc/eltwise.hip dmy_image_s2d / dmy_nchw_to_nhwc, csrc/tta.hip)."""
import math

import torch

from .._lib import call, ptr, stream
from ._base import CL, DT, dcode, pixel_stride, vec_pad


def _image_src(x):
    """-> (contiguous source, kind, scale) of an NCHW image for the image kernels: uint8 (kind 0) is scaled by 1 / 255,
    any float image is read as fp32 (kind 1) unscaled"""
    xc = x.contiguous()
    if x.dtype == torch.uint8:
        return xc, 0, 1.0 / 255.0
    return (xc if xc.dtype == torch.float32 else xc.float()), 1, 1.0


def image_s2d(x, dtype):
    """NCHW image (uint8 -> /255, or float) -> space-to-depth NHWC storage [N, Cs, H/2, W/2] for the k6 s2 p2
    stem (csrc dmy_image_s2d); the result carries `_dmy_s2d` = C, read by ConvBNActFn.  No gradient."""
    N, C, H, W = x.shape
    Cs = vec_pad(4 * C, dtype)
    buf = torch.empty((N, Cs, H // 2, W // 2), dtype=dtype, device=x.device, memory_format=CL)
    src, kind, scale = _image_src(x.detach())
    call('dmy_image_s2d', DT[dtype], kind, ptr(src), ptr(buf), N, C, H, W, Cs, scale, stream())
    buf._dmy_s2d = C
    return buf


def tta_image(x, dtype, ratio, flip, gs, s2d):
    """One test-time-augmentation input (models/yolo.py:201: scale_img(x.flip(flip) if flip else x, ratio, gs=gs),
    utils/torch_utils.py:264-274) as the stem's input, in one launch (csrc dmy_tta_image): NCHW uint8 (/255) or float
    image -> flip (None / 0, 2 up-down, 3 left-right) -> bilinear resize to (int(H*ratio), int(W*ratio)) -> 0.447 pad to
    the next gs multiple -> `dtype` in NHWC storage, space-to-depth (`_dmy_s2d`, as image_s2d) or channel-padded
    (`_dmy_cpad`, as Model.to_input's ToNHWC).  No gradient."""
    N, C, H, W = x.shape
    flip = int(flip or 0)
    if ratio == 1.0:
        OH, OW, OHp, OWp = H, W, H, W
    else:
        OH, OW = int(H * ratio), int(W * ratio)
        OHp, OWp = (math.ceil(v * ratio / gs) * gs for v in (H, W))
    xc, kind, scale = _image_src(x.detach())
    if s2d:
        Cs = vec_pad(4 * C, dtype)
        buf = torch.empty((N, Cs, OHp // 2, OWp // 2), dtype=dtype, device=x.device, memory_format=CL)
    else:
        Cs = vec_pad(C, dtype)
        buf = torch.empty((N, Cs, OHp, OWp), dtype=dtype, device=x.device, memory_format=CL)
    call('dmy_tta_image', DT[dtype], kind, ptr(xc), ptr(buf), N, C, H, W, int(bool(s2d)), Cs, scale, flip, OH, OW, OHp,
         OWp, 0.447, stream())
    if s2d:
        buf._dmy_s2d = C
        return buf
    y = buf[:, :C] if Cs != C else buf
    y._dmy_cpad = Cs
    return y


class ToNHWC(torch.autograd.Function):
    """NCHW float/uint8 image -> NHWC storage dtype (train.py:402 `/255` when uint8).  The pixel
    stride is rounded up to a 16-byte vector with zero channels so the stem conv stays vectorised."""

    @staticmethod
    def forward(ctx, x, dtype):
        N, C, H, W = x.shape
        Cp = vec_pad(C, dtype)
        buf = torch.empty((N, Cp, H, W), dtype=dtype, device=x.device, memory_format=CL)
        src, kind, scale = _image_src(x)  # not detached: forward runs with grad off
        call('dmy_nchw_to_nhwc', DT[dtype], kind, ptr(src), ptr(buf), N, C, H, W, Cp, scale, stream())
        ctx.src_dtype = x.dtype
        ctx.mark_non_differentiable(buf) if x.dtype == torch.uint8 else None
        return buf[:, :C] if Cp != C else buf

    @staticmethod
    def backward(ctx, dy):
        if ctx.src_dtype == torch.uint8:
            return None, None
        dy, dps = pixel_stride(dy)
        N, C, H, W = dy.shape
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
        call('dmy_nhwc_to_nchw_f32', dcode(dy), ptr(dy), dps, ptr(dx), N, C, H, W, stream())
        return dx.to(ctx.src_dtype), None
