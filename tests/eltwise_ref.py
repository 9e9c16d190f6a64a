"""Plain-torch fp64 restatement of the operations behind csrc/eltwise.hip's gating / attention / layout kernels and
csrc/swin.hip's LayerNorm (TEST INFRASTRUCTURE ONLY, like tests/hor_ref.py).  Written from the formulas, not from the
kernels; tests/test_eltwise_ref.py checks every function here against fp64 autograd of the plain torch ops.

Conventions
* activations are NHWC tensors [N, H, W, C] (or [N, HW, C] / [M, C]) of fp64 values that are exact in the storage type
  under test; `dtype` is that storage type (torch.float32 / torch.bfloat16)
* a storage rounding point that a kernel documents as part of its contract is `rnd(t, dtype)` and nothing else
* every function returns, next to each output, the absolute sum of the terms that feed it (sum |term|): the error bound
  of an fp32 evaluation is a multiple of 2^-24 of that sum (see `bound`)
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24      # fp32 unit roundoff
BF16_STORE = 2.0 ** -8  # one rounding to bf16 storage, relative (half an ulp of a bf16 value is at most 2^-8 of it)
TRANS = 1e-5          # the project's fp32 elementwise tolerance (tests/test_gpu_pools.py), rtol = atol


def rnd(t, dtype):
    return t.to(dtype).double()


def bound(ref, abssum, n, dtype_out, trans=False):
    """|out - ref| allowed for an fp32 evaluation of `n` operations / terms with absolute term sum `abssum`:
    n * 2^-24 * sum|term|  (n = 4 for an elementwise expression of a handful of operations, n = the number of terms of a
    sequential sum) + rtol = atol = 1e-5 when the value passes through sigmoid / rsqrt / erf + one storage rounding when
    the output is stored in bf16."""
    b = n * U32 * abssum
    if trans:
        b = b + TRANS * (1.0 + ref.abs())
    if dtype_out == torch.bfloat16:
        b = b + BF16_STORE * ref.abs()
    return b


# ---------------------------------------------------------------- avg-pool r x r, stride r, floor mode
def avgpool_fwd(x, r):
    N, H, W, C = x.shape
    OH, OW = H // r, W // r
    v = x[:, :OH * r, :OW * r].reshape(N, OH, r, OW, r, C)
    return v.mean((2, 4)), v.abs().sum((2, 4)) / (r * r)


def avgpool_bwd(dy, H, W, r):
    N, OH, OW, C = dy.shape
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    dx[:, :OH * r, :OW * r] = dy.repeat_interleave(r, 1).repeat_interleave(r, 2) / (r * r)
    return dx, dx.abs()


# ---------------------------------------------------------------- nearest resize
def nearest_index(n_in, n_out):
    """ATen's nearest rule: src = min(floor(dst * scale), in - 1) with scale = in / out evaluated in fp32"""
    if n_in == n_out:
        return torch.arange(n_out)
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    d = torch.arange(n_out, dtype=torch.float32)
    return torch.clamp(torch.floor(d * scale).long(), max=n_in - 1)


def resize_fwd(x, OH, OW, yscale=1.0):
    ih, iw = nearest_index(x.shape[1], OH), nearest_index(x.shape[2], OW)
    y = x[:, ih][:, :, iw] * yscale
    return y, y.abs()


def resize_bwd(dy, IH, IW):
    N, OH, OW, C = dy.shape
    ih, iw = nearest_index(IH, OH), nearest_index(IW, OW)

    def fold(t):
        a = torch.zeros(N, IH, OW, C, dtype=torch.float64).index_add_(1, ih, t)
        return torch.zeros(N, IH, IW, C, dtype=torch.float64).index_add_(2, iw, a)
    return fold(dy), fold(dy.abs())


def resize_max_preimage(IH, IW, OH, OW):
    """the largest number of output pixels that map to one input pixel (terms of one resize_bwd sum)"""
    ih, iw = nearest_index(IH, OH), nearest_index(IW, OW)
    return int(torch.bincount(ih).max()) * int(torch.bincount(iw).max())


# ---------------------------------------------------------------- SCConv gate: out = u3 * sigmoid(x + nearest(g))
def scgate_pre(x, g, dtype):
    N, H, W, C = x.shape
    gu = g[:, nearest_index(g.shape[1], H)][:, :, nearest_index(g.shape[2], W)]
    return rnd(x + gu, dtype)   # documented rounding: the sum is stored before the sigmoid


def scgate_fwd(x, u3, g, dtype):
    """-> out, the sigmoid before its (documented) storage rounding, sum|term|"""
    s = torch.sigmoid(scgate_pre(x, g, dtype))
    out = u3 * rnd(s, dtype)
    return out, s, out.abs()


def scgate_bwd(x, u3, g, dout, dtype):
    """du3 = dout * s, dpre = dout * u3 * s (1 - s)  with s = sigmoid(rnd(x + up(g)))"""
    s = torch.sigmoid(scgate_pre(x, g, dtype))
    du3 = dout * s
    dpre = dout * u3 * s * (1 - s)
    return du3, dpre, du3.abs(), dpre.abs()


# ---------------------------------------------------------------- CoorAttention
def ca_pool_fwd(x):
    """[N, H, W, C] -> [N, H + W, C]: means over w, then means over h"""
    y = torch.cat([x.mean(2), x.mean(1)], 1)
    a = torch.cat([x.abs().mean(2), x.abs().mean(1)], 1)
    return y, a


def ca_pool_bwd(dy, H, W):
    a = dy[:, :H, None, :] / W
    b = dy[:, None, H:, :] / H
    return a + b, a.abs() + b.abs()


def ca_att(lh, lw, H):
    return torch.sigmoid(lh[:, :H, None, :]), torch.sigmoid(lw[:, None, H:, :])


def ca_apply_fwd(x, lh, lw):
    ah, aw = ca_att(lh, lw, x.shape[1])
    out = x * aw * ah
    return out, out.abs()


def ca_apply_bwd(x, lh, lw, dout):
    """-> dx, dlh, dlw and their sum|term|; dlh / dlw are [N, H + W, C] with the other operand's rows zero"""
    H = x.shape[1]
    ah, aw = ca_att(lh, lw, H)
    dx = dout * aw * ah
    th = dout * x * aw * ah * (1 - ah)       # summed over w
    tw = dout * x * ah * aw * (1 - aw)       # summed over h
    zh, zw = torch.zeros_like(lh[:, H:]), torch.zeros_like(lh[:, :H])
    dlh = torch.cat([th.sum(2), zh], 1)
    dlw = torch.cat([zw, tw.sum(1)], 1)
    alh = torch.cat([th.abs().sum(2), zh], 1)
    alw = torch.cat([zw, tw.abs().sum(1)], 1)
    return dx, dlh, dlw, dx.abs(), alh, alw


# ---------------------------------------------------------------- CBAM
def halves_sigmoid_fwd(z, dtype):
    """z [2N, C] -> sigmoid(rnd(z[:N] + z[N:]))  (documented rounding: the sum of the halves is stored)"""
    N = z.shape[0] // 2
    return torch.sigmoid(rnd(z[:N] + z[N:], dtype))


def halves_sigmoid_bwd(z, dca, dtype):
    s = halves_sigmoid_fwd(z, dtype)
    g = dca * s * (1 - s)
    return torch.cat([g, g], 0)


def cbam_in_fwd(x, ca, dtype):
    """x [N, HW, C], ca [N, C] -> out1 = rnd(x * ca) (documented rounding), its channel mean, channel max, the first
    argmax channel, and sum|term| of the mean"""
    out1 = rnd(x * ca[:, None, :], dtype)
    mx = out1.max(-1)[0]
    am = (out1 == mx[..., None]).int().argmax(-1)   # argmax returns the first of several maxima
    return out1, out1.mean(-1), mx, am, out1.abs().mean(-1)


def cbam_in_bwd(x, ca, dout1, ds2, am):
    """ds2 [N, HW, 2] = (d mean, d max) -> dx, dca and sum|term| of each"""
    C = x.shape[-1]
    hot = F.one_hot(am, C).double()
    gm, gx = ds2[..., :1] / C, ds2[..., 1:] * hot
    t = dout1 + gm + gx
    ta = dout1.abs() + gm.abs() + gx.abs()
    dx = t * ca[:, None, :]
    return dx, (t * x).sum(1), ta * ca[:, None, :].abs(), (ta * x.abs()).sum(1)


def pixscale_fwd(out1, sa):
    out = out1 * sa[..., None]
    return out, out.abs()


def pixscale_bwd(out1, sa, dout):
    d1 = dout * sa[..., None]
    return d1, (dout * out1).sum(-1), d1.abs(), (dout * out1).abs().sum(-1)


# ---------------------------------------------------------------- LayerNorm over channels, x [M, C]
def layernorm_fwd(x, w, b, eps):
    """-> y, mean, rstd, sum|term| of y's last affine step, sum|term| of the mean"""
    C = x.shape[1]
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(1) + eps)
    xh = d * rstd[:, None]
    return xh * w + b, mean, rstd, (xh * w).abs() + b.abs(), x.abs().sum(1) / C


def layernorm_bwd(x, dy, w, mean, rstd):
    """the backward as a function of the saved fp32 statistics (inputs of the backward kernel):
    dx = rstd (g - mean_c g - xhat mean_c (g xhat)), g = dy w; dw = sum_m dy xhat; db = sum_m dy.
    -> dx, dw, db, sum|term| of dx (before the rstd factor is applied: already multiplied by it), of the two row means
    a1 = mean g and a2 = mean (g xhat), of dw and of db"""
    C = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    a1, a2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (g - a1 - xh * a2)
    r = rstd[:, None].abs()
    adx = r * (g.abs() + a1.abs() + (xh * a2).abs())
    aa1 = r * g.abs().sum(1, keepdim=True) / C
    aa2 = r * xh.abs() * (g * xh).abs().sum(1, keepdim=True) / C
    return dx, (dy * xh).sum(0), dy.sum(0), adx, aa1, aa2, (dy * xh).abs().sum(0), dy.abs().sum(0)


# ---------------------------------------------------------------- layout / pointwise
def nchw_to_nhwc(x, Cp, scale):
    """x [N, C, H, W] (uint8 or fp32) -> [N, H, W, Cp] fp64 with zero channels [C, Cp); `scale` is an fp32 number"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, Cp, dtype=torch.float64)
    y[..., :C] = x.double().permute(0, 2, 3, 1) * float(torch.tensor(scale, dtype=torch.float32))
    return y


def nhwc_to_nchw(x):
    return x.double().permute(0, 3, 1, 2).contiguous()


ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_SIGMOID, ACT_GELU, ACT_RELU, ACT_LEAKY = range(7)
ACT_TRANS = (ACT_SILU, ACT_SIGMOID, ACT_GELU)   # pass through sigmoid / erf / exp


def act(code, u):
    """-> act(u), sum|term|"""
    if code == ACT_SILU:
        y = u * torch.sigmoid(u)
    elif code == ACT_HARDSWISH:
        return u * torch.clamp(u + 3, 0, 6) / 6, u.abs() * (u.abs() + 3) / 6
    elif code == ACT_SIGMOID:
        y = torch.sigmoid(u)
    elif code == ACT_GELU:
        y = 0.5 * u * (1 + torch.erf(u / 2 ** 0.5))
    elif code == ACT_RELU:
        y = torch.clamp(u, min=0)
    elif code == ACT_LEAKY:
        y = torch.where(u > 0, u, 0.1 * u)
    else:
        y = u.clone()
    return y, y.abs()


def act_grad(code, u):
    """-> d act / d u with torch's backward conventions at the kinks, sum|term|"""
    one = torch.ones_like(u)
    if code == ACT_SILU:
        s = torch.sigmoid(u)
        d = s * (1 + u * (1 - s))
        return d, s * (1 + (u * (1 - s)).abs())
    if code == ACT_HARDSWISH:   # hardswish_backward: u <= -3 -> 0, u < 3 -> u / 3 + 0.5, else 1
        d = torch.where(u <= -3, 0 * one, torch.where(u < 3, u / 3 + 0.5, one))
        return d, torch.where(u <= -3, 0 * one, torch.where(u < 3, u.abs() / 3 + 0.5, one))
    if code == ACT_SIGMOID:
        s = torch.sigmoid(u)
        return s * (1 - s), s * (1 - s)
    if code == ACT_GELU:
        a = 0.5 * (1 + torch.erf(u / 2 ** 0.5))
        b = u * torch.exp(-0.5 * u * u) / (2 * torch.pi) ** 0.5
        return a + b, a.abs() + b.abs()
    if code == ACT_RELU:        # threshold_backward: u > 0
        d = (u > 0).double()
        return d, d
    if code == ACT_LEAKY:       # leaky_relu_backward: u > 0 ? 1 : slope
        d = torch.where(u > 0, one, 0.1 * one)
        return d, d
    return one, one


def pointwise(op, code, a, b, alpha):
    """op: 0 a + b, 1 act(a), 2 b * act'(a), 3 a * alpha, 4 a + alpha * b  -> y, sum|term|"""
    if op == 0:
        return a + b, a.abs() + b.abs()
    if op == 1:
        return act(code, a)
    if op == 2:
        d, ad = act_grad(code, a)
        return b * d, b.abs() * ad
    if op == 3:
        return a * alpha, (a * alpha).abs()
    return a + alpha * b, a.abs() + (alpha * b).abs()
