"""CPU: every function of tests/eltwise_ref.py against fp64 autograd of the plain torch ops (F.avg_pool2d,
F.interpolate(mode='nearest'), F.layer_norm, the CoorAttention / CBAM / SCConv expressions of oracle/nn.py, permute),
so the GPU tests (tests/test_gpu_eltwise.py, tests/test_gpu_layernorm.py) do not trust an unchecked restatement."""
import pytest
import torch
import torch.nn.functional as F

import eltwise_ref as R

RTOL, ATOL = 1e-12, 1e-12
F32 = torch.float32


def close(a, b):
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('r', [2, 4])
@pytest.mark.parametrize('N,H,W,C', [(2, 9, 14, 6), (1, 17, 23, 5), (2, 8, 8, 4)])
def test_avgpool(r, N, H, W, C):
    x = rand(N, H, W, C, seed=r + H).requires_grad_(True)
    y = nhwc(F.avg_pool2d(nchw(x), r, r))
    dy = rand(*y.shape, seed=1)
    y.backward(dy)
    yr, ya = R.avgpool_fwd(x.detach(), r)
    close(yr, y.detach())
    close(ya, nhwc(F.avg_pool2d(nchw(x.detach().abs()), r, r)))
    dx, da = R.avgpool_bwd(dy, H, W, r)
    close(dx, x.grad)
    close(da, x.grad.abs())
    assert bool((dx[:, (H // r) * r:] == 0).all()) and bool((dx[:, :, (W // r) * r:] == 0).all())


RESIZES = [((5, 7), (10, 14)), ((5, 7), (5, 7)), ((5, 7), (13, 20)), ((4, 5), (17, 23)), ((13, 20), (5, 7))]


@pytest.mark.parametrize('src,dst', RESIZES)
def test_resize(src, dst):
    (IH, IW), (OH, OW) = src, dst
    # the index map itself, from the fp32 op the models run (indices as values) and from the fp64 one
    idx = torch.arange(IH * IW, dtype=F32).view(1, 1, IH, IW)
    want = F.interpolate(idx, size=dst, mode='nearest').long().view(OH, OW)
    got = R.nearest_index(IH, OH)[:, None] * IW + R.nearest_index(IW, OW)[None, :]
    assert torch.equal(got, want)
    assert torch.equal(F.interpolate(idx.double(), size=dst, mode='nearest').long().view(OH, OW), want)
    x = rand(2, IH, IW, 3, seed=OH).requires_grad_(True)
    y = nhwc(F.interpolate(nchw(x), size=dst, mode='nearest')) * 0.5
    dy = rand(*y.shape, seed=2)
    y.backward(dy)
    yr, ya = R.resize_fwd(x.detach(), OH, OW, 0.5)
    close(yr, y.detach())
    close(ya, y.detach().abs())
    dx, da = R.resize_bwd(dy, IH, IW)
    close(dx, x.grad / 0.5)
    ones = R.resize_bwd(torch.ones(1, OH, OW, 1, dtype=torch.float64), IH, IW)[0]
    assert int(ones.max()) == R.resize_max_preimage(IH, IW, OH, OW) and float(ones.sum()) == OH * OW
    assert bool((da >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize('H,W,GH,GW', [(16, 16, 4, 4), (17, 23, 4, 5), (9, 6, 2, 1)])
@pytest.mark.parametrize('dtype', [torch.float64, torch.bfloat16])
def test_scgate(H, W, GH, GW, dtype):
    """oracle.nn.SCConv.forward's gate expression: k3(x) * sigmoid(x + interpolate(k2(x)))"""
    gen = torch.Generator().manual_seed(H)
    x = (torch.randint(-64, 65, (2, H, W, 3), generator=gen).double() / 16).requires_grad_(True)
    g = (torch.randint(-64, 65, (2, GH, GW, 3), generator=gen).double() / 16).requires_grad_(True)
    u3 = rand(2, H, W, 3, seed=1).requires_grad_(True)
    dout = rand(2, H, W, 3, seed=2)
    s = torch.sigmoid(x + nhwc(F.interpolate(nchw(g), size=(H, W), mode='nearest')))
    out, sr, oa = R.scgate_fwd(x.detach(), u3.detach(), g.detach(), dtype)
    close(sr, s.detach())                      # x + g is exact on the grid: the rounding of the sum is the identity
    close(out, u3.detach() * R.rnd(s.detach(), dtype))
    close(oa, out.abs())
    (u3 * s).backward(dout)
    du3, dpre, a3, ap = R.scgate_bwd(x.detach(), u3.detach(), g.detach(), dout, dtype)
    close(du3, u3.grad)
    close(dpre, x.grad)
    close(R.resize_bwd(dpre, GH, GW)[0], g.grad)   # the gate's g gradient is the resize backward of dpre
    close(a3, du3.abs())
    close(ap, dpre.abs())


@pytest.mark.parametrize('N,H,W,C', [(2, 5, 9, 6), (1, 12, 3, 4), (3, 1, 7, 3)])
def test_coorattention(N, H, W, C):
    """oracle.nn.CoorAttention.forward: cat(x.mean(3), x.mean(2)) and x * a_w * a_h"""
    x = rand(N, H, W, C, seed=H).requires_grad_(True)
    xc = nchw(x)
    pooled = torch.cat([xc.mean(3, keepdim=True), xc.mean(2, keepdim=True).transpose(2, 3)], 2)  # [N, C, H + W, 1]
    dy = rand(N, H + W, C, seed=1)
    pooled.backward(dy.permute(0, 2, 1)[..., None])
    y, ya = R.ca_pool_fwd(x.detach())
    close(y, pooled.detach()[..., 0].permute(0, 2, 1))
    close(ya, R.ca_pool_fwd(x.detach().abs())[0])
    dx, da = R.ca_pool_bwd(dy, H, W)
    close(dx, x.grad)
    assert bool((da >= dx.abs() - 1e-12).all())

    x.grad = None
    lh = rand(N, H + W, C, seed=2).requires_grad_(True)
    lw = rand(N, H + W, C, seed=3).requires_grad_(True)
    ah = torch.sigmoid(lh[:, :H].permute(0, 2, 1)[..., None])         # [N, C, H, 1]
    aw = torch.sigmoid(lw[:, H:].permute(0, 2, 1)[:, :, None, :])     # [N, C, 1, W]
    out = xc * aw * ah
    dout = rand(N, H, W, C, seed=4)
    out.backward(nchw(dout))
    o, oa = R.ca_apply_fwd(x.detach(), lh.detach(), lw.detach())
    close(o, nhwc(out.detach()))
    close(oa, o.abs())
    dxr, dlh, dlw, _, alh, alw = R.ca_apply_bwd(x.detach(), lh.detach(), lw.detach(), dout)
    close(dxr, x.grad)
    close(dlh, lh.grad)
    close(dlw, lw.grad)
    assert bool((dlh[:, H:] == 0).all()) and bool((dlw[:, :H] == 0).all())
    assert bool((alh >= dlh.abs() - 1e-12).all()) and bool((alw >= dlw.abs() - 1e-12).all())


@pytest.mark.parametrize('N,HW,C', [(1, 7, 6), (3, 70, 16)])
def test_cbam(N, HW, C):
    """oracle.nn.CBAM: sigmoid(a + m), out1 = ca * x, cat(mean_c out1, max_c out1), sa * out1"""
    z = rand(2 * N, C, seed=HW).requires_grad_(True)
    ca = torch.sigmoid(z[:N] + z[N:])
    dca = rand(N, C, seed=1)
    ca.backward(dca)
    close(R.halves_sigmoid_fwd(z.detach(), torch.float64), ca.detach())
    dz = R.halves_sigmoid_bwd(z.detach(), dca, torch.float64)
    close(dz, z.grad)
    assert torch.equal(dz[:N], dz[N:])

    x = rand(N, HW, C, seed=2).requires_grad_(True)
    cav = ca.detach().clone().requires_grad_(True)
    out1 = x * cav[:, None, :]
    mx, idx = out1.max(-1)
    s2 = torch.stack([out1.mean(-1), mx], -1)
    d1, ds2 = rand(N, HW, C, seed=3), rand(N, HW, 2, seed=4)
    torch.autograd.backward([out1, s2], [d1, ds2])
    o1, mean, mxr, am, ma = R.cbam_in_fwd(x.detach(), cav.detach(), torch.float64)
    close(o1, out1.detach())
    close(mean, s2.detach()[..., 0])
    assert torch.equal(mxr, mx.detach()) and torch.equal(am, idx)
    close(ma, out1.detach().abs().mean(-1))
    dx, dcar, xa, caa = R.cbam_in_bwd(x.detach(), cav.detach(), d1, ds2, am)
    close(dx, x.grad)
    close(dcar, cav.grad)
    assert bool((xa >= dx.abs() - 1e-12).all()) and bool((caa >= dcar.abs() - 1e-12).all())
    # ties: the first channel wins
    xt = torch.ones(1, 2, 4, dtype=torch.float64)
    assert R.cbam_in_fwd(xt, torch.ones(1, 4, dtype=torch.float64), torch.bfloat16)[3].tolist() == [[0, 0]]

    o = o1.clone().requires_grad_(True)
    sa = rand(N, HW, seed=5).requires_grad_(True)
    out = o * sa[..., None]
    dout = rand(N, HW, C, seed=6)
    out.backward(dout)
    close(R.pixscale_fwd(o.detach(), sa.detach())[0], out.detach())
    g1, gsa, _, sab = R.pixscale_bwd(o.detach(), sa.detach(), dout)
    close(g1, o.grad)
    close(gsa, sa.grad)
    assert bool((sab >= gsa.abs() - 1e-12).all())


@pytest.mark.parametrize('M,C', [(1, 7), (37, 24), (67, 260)])
@pytest.mark.parametrize('eps', [1e-5, 1e-6])
def test_layernorm(M, C, eps):
    x = (rand(M, C, seed=C) * 0.7 + 0.3).requires_grad_(True)
    w = (rand(C, seed=1) * 0.5 + 1).requires_grad_(True)
    b = rand(C, seed=2).requires_grad_(True)
    y = F.layer_norm(x, (C,), w, b, eps)
    dy = rand(M, C, seed=3)
    y.backward(dy)
    yr, mean, rstd, ya, ma = R.layernorm_fwd(x.detach(), w.detach(), b.detach(), eps)
    close(yr, y.detach())
    close(mean, x.detach().mean(1))
    close(rstd, torch.rsqrt(x.detach().var(1, unbiased=False) + eps))
    close(ma, x.detach().abs().mean(1))
    assert bool((ya >= yr.abs() - 1e-12).all())
    dx, dw, db, adx, aa1, aa2, adw, adb = R.layernorm_bwd(x.detach(), dy, w.detach(), mean, rstd)
    close(dx, x.grad)
    close(dw, w.grad)
    close(db, b.grad)
    assert bool((adx >= dx.abs() - 1e-12).all())
    assert bool((adw >= dw.abs() - 1e-12).all()) and bool((adb >= db.abs() - 1e-12).all())
    assert bool((aa1 >= 0).all()) and bool((aa2 >= 0).all())


def test_layout():
    x8 = torch.randint(0, 256, (2, 3, 5, 7), dtype=torch.uint8)
    y = R.nchw_to_nhwc(x8, 8, 1.0 / 255.0)
    close(y[..., :3], x8.double().permute(0, 2, 3, 1) * float(torch.tensor(1 / 255.0, dtype=F32)))
    assert bool((y[..., 3:] == 0).all()) and tuple(y.shape) == (2, 5, 7, 8)
    xf = rand(2, 5, 7, 4).float()
    assert torch.equal(R.nhwc_to_nchw(xf), xf.double().permute(0, 3, 1, 2))
    assert torch.equal(R.nhwc_to_nchw(R.nchw_to_nhwc(xf.permute(0, 3, 1, 2), 4, 1.0)), xf.double().permute(0, 3, 1, 2))


TORCH_ACT = {R.ACT_NONE: lambda u: u * 1, R.ACT_SILU: F.silu, R.ACT_HARDSWISH: F.hardswish, R.ACT_SIGMOID: torch.sigmoid,
             R.ACT_GELU: F.gelu, R.ACT_RELU: F.relu, R.ACT_LEAKY: lambda u: F.leaky_relu(u, 0.1)}


@pytest.mark.parametrize('code', sorted(TORCH_ACT))
def test_activations(code):
    u = torch.cat([torch.tensor([-3.0, 3.0, 0.0, -0.0, -8.0, 8.0], dtype=torch.float64), rand(300) * 3]).requires_grad_(True)
    y = TORCH_ACT[code](u)
    dy = rand(u.numel(), seed=1)
    y.backward(dy)
    yr, ya = R.pointwise(1, code, u.detach(), None, 0.0)
    close(yr, y.detach())
    assert bool((ya >= yr.abs() - 1e-12).all())
    gr, ga = R.pointwise(2, code, u.detach(), dy, 0.0)
    close(gr, u.grad)   # includes torch's conventions at hardswish +-3, relu / leaky 0
    assert bool((ga >= gr.abs() - 1e-12).all())


def test_pointwise_linear_ops():
    a, b = rand(50, seed=1), rand(50, seed=2)
    close(R.pointwise(0, 0, a, b, 0.0)[0], a + b)
    close(R.pointwise(3, 0, a, b, 0.3)[0], a * 0.3)
    close(R.pointwise(4, 0, a, b, 0.3)[0], a + 0.3 * b)


def test_bound():
    ref, s = torch.tensor([2.0], dtype=torch.float64), torch.tensor([3.0], dtype=torch.float64)
    assert float(R.bound(ref, s, 4, F32)) == 4 * 2.0 ** -24 * 3.0
    assert float(R.bound(ref, s, 4, torch.bfloat16)) == 4 * 2.0 ** -24 * 3.0 + 2.0 ** -8 * 2.0
    assert float(R.bound(ref, s, 4, F32, trans=True)) == 4 * 2.0 ** -24 * 3.0 + 1e-5 * 3.0
