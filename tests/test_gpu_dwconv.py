"""GPU: the depthwise conv kernels (csrc/dwconv.hip) through the C ABI against F.conv2d(groups=C),
torch.nn.grad.conv2d_input and conv2d_weight in fp32 on the same storage-rounded operands.  Bounds are those of
tests/test_gpu_conv.py for the dense kernels' same comparisons (output / data-grad rel-L2 < 1e-2, partial sums 1e-3,
weight-grad 2e-3).  The BN partial rows are sums of the values AS STORED (include/dmayolo.h), so their reference is the
reference output rounded to the storage dtype."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOMS = [(5, 1), (3, 1), (3, 2)]  # (k, s), p = k // 2
# (N, C, H, W, Ct, c0): one vector + odd sizes; several pixel blocks + ragged channel tile (3 vectors in a tile of 4);
# image smaller than the 5x5 filter; even sizes under stride 2; channel slices [16:32] of 48-channel buffers
SHAPES = [(2, 8, 13, 17, 8, 0), (3, 24, 33, 37, 24, 0), (1, 40, 3, 4, 40, 0), (2, 64, 16, 16, 64, 0),
          (2, 16, 9, 11, 48, 16)]
CL = torch.channels_last


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12))


def _slice(t, Ct, c0, fill=float('nan')):
    """t (N, C, H, W) placed in channels [c0, c0 + C) of a (N, Ct, H, W) NHWC buffer filled with `fill`"""
    N, C, H, W = t.shape
    buf = torch.full((N, Ct, H, W), fill, dtype=t.dtype, device='cuda').contiguous(memory_format=CL)
    v = buf[:, c0:c0 + C]
    v.copy_(t)
    return buf, v


def _others_untouched(buf, C, c0):
    rest = torch.cat([buf[:, :c0], buf[:, c0 + C:]], 1)
    return rest.numel() == 0 or bool(torch.isnan(rest).all())


def _case(N, C, H, W, k, s, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    p = k // 2
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    w = torch.randn(C, 1, k, k, generator=g) / k
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dz = torch.randn(N, C, OH, OW, generator=g).to(dtype)
    return x, w, dz, p, OH, OW


def _wop(w, dtype):
    from dmayolo.functional import prep_weight
    return prep_weight(w.cuda(), dtype, True)[1]  # the IHWO copy of (C, 1, k, k) == [k][k][C]


@pytest.mark.parametrize('k,s', GEOMS)
@pytest.mark.parametrize('N,C,H,W,Ct,c0', SHAPES)
def test_dwconv_fwd_bf16_vs_torch(N, C, H, W, Ct, c0, k, s):
    from dmayolo.functional import call, ptr, stream
    x, w, _, p, OH, OW = _case(N, C, H, W, k, s, 100 * N + C + k + s)
    ref = F.conv2d(x.float().cuda(), w.bfloat16().float().cuda(), stride=s, padding=p, groups=C)
    xb, xv = _slice(x.cuda(), Ct, c0)
    zb, zv = _slice(torch.zeros(N, C, OH, OW, dtype=torch.bfloat16), Ct, c0)
    zv.fill_(float('nan'))
    wd = _wop(w, torch.bfloat16)
    M = N * OH * OW
    assert call('dmy_dwconv_ok', 1, ptr(xv), ptr(wd), ptr(zv), N, H, W, C, C, C, Ct, k, k, s, p, OH, OW, Ct) == 1
    P = call('dmy_dwconv_fwd_rows', M, C)
    ps = torch.full((P, C), float('nan'), device='cuda')
    pq = torch.full((P, C), float('nan'), device='cuda')
    call('dmy_dwconv_fwd', 1, ptr(xv), ptr(wd), None, ptr(zv), ptr(ps), ptr(pq), N, H, W, C, Ct, k, k, s, p, OH, OW, Ct,
         stream())
    torch.cuda.synchronize()
    assert _others_untouched(zb, C, c0) and _others_untouched(xb, C, c0)
    assert torch.isfinite(zv).all()
    assert _rel(zv.float(), ref) < 1e-2
    assert torch.isfinite(ps).all() and torch.isfinite(pq).all(), 'every partial row must be written'
    stored = ref.bfloat16().double()
    s1, s2 = stored.sum((0, 2, 3)), (stored ** 2).sum((0, 2, 3))
    e1, e2 = _rel(ps.sum(0), s1), _rel(pq.sum(0), s2)
    print(f'fwd {N, C, H, W} k{k} s{s}: y {_rel(zv.float(), ref):.2e} psum {e1:.2e} psq {e2:.2e} rows {P}')
    assert e1 < 1e-3 or float((ps.sum(0).double() - s1).abs().max()) < 1e-2 * M ** 0.5
    assert e2 < 1e-3


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('k,s', GEOMS)
@pytest.mark.parametrize('N,C,H,W,Ct,c0', SHAPES)
def test_dwconv_dgrad_bf16_vs_torch(N, C, H, W, Ct, c0, k, s, acc):
    from dmayolo.functional import call, ptr, stream
    x, w, dz, p, OH, OW = _case(N, C, H, W, k, s, 100 * N + C + k + s + 7)
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.bfloat16().float().cuda(), dz.float().cuda(), stride=s, padding=p,
                                     groups=C)
    if acc:
        ref = ref + x.float().cuda()  # x doubles as the previous dx
    db, dv = _slice(x.cuda(), Ct, c0)
    if not acc:
        dv.fill_(float('nan'))
    zb, zv = _slice(dz.cuda(), Ct, c0)
    call('dmy_dwconv_dgrad', 1, ptr(zv), ptr(_wop(w, torch.bfloat16)), ptr(dv), acc, N, H, W, C, Ct, k, k, s, p, OH, OW,
         Ct, stream())
    torch.cuda.synchronize()
    assert _others_untouched(db, C, c0)
    assert torch.isfinite(dv).all()
    assert _rel(dv.float(), ref) < 1e-2, _rel(dv.float(), ref)


@pytest.mark.parametrize('k,s', GEOMS)
@pytest.mark.parametrize('N,C,H,W,Ct,c0', SHAPES)
def test_dwconv_wgrad_bf16_vs_torch(N, C, H, W, Ct, c0, k, s):
    from dmayolo.functional import call, ptr, stream
    x, _, dz, p, OH, OW = _case(N, C, H, W, k, s, 100 * N + C + k + s + 11)
    ref = torch.nn.grad.conv2d_weight(x.float().cuda(), (C, 1, k, k), dz.float().cuda(), stride=s, padding=p, groups=C)
    _, xv = _slice(x.cuda(), Ct, c0)
    _, zv = _slice(dz.cuda(), Ct, c0)
    P = call('dmy_dwconv_wgrad_rows', N * OH * OW, C)
    outs = []
    for run in range(2):
        part = torch.full((P, k * k * C), float('nan'), device='cuda')
        dw = torch.full((C, 1, k, k), float('nan'), device='cuda')
        call('dmy_dwconv_wgrad', 1, ptr(xv), ptr(zv), ptr(part), N, H, W, C, Ct, k, k, s, p, OH, OW, Ct, stream())
        call('dmy_dwconv_wgrad_finalize', ptr(part), P, C, k, k, ptr(dw), 0, stream())
        torch.cuda.synchronize()
        assert torch.isfinite(part).all(), 'every partial row must be written'
        outs.append(dw)
    assert _rel(outs[0], ref) < 2e-3, _rel(outs[0], ref)
    assert torch.equal(outs[0], outs[1])  # no atomics: bit-identical run to run
    acc = torch.ones(C, 1, k, k, device='cuda')
    call('dmy_dwconv_wgrad_finalize', ptr(part), P, C, k, k, ptr(acc), 1, stream())
    torch.cuda.synchronize()
    assert torch.equal(acc, 1 + outs[0])


@pytest.mark.parametrize('k,s', GEOMS)
@pytest.mark.parametrize('N,C,H,W,Ct,c0', SHAPES)
def test_dwconv_fp32_storage(N, C, H, W, Ct, c0, k, s):
    """fp32 storage: each kernel may differ from a float64 computation by 4x what torch's own fp32 depthwise conv
    differs from it on the same inputs (the factor covers the accumulation order of at most 49 terms).  Measured on the
    MI355X over these 15 cases, rel-L2 against float64, torch | kernel: forward 4.2e-8 .. 9.0e-8 | 4.1e-8 .. 9.1e-8,
    data-grad 3.8e-8 .. 9.5e-8 | 3.3e-8 .. 8.9e-8, weight-grad 3.3e-8 .. 4.6e-7 | 3.5e-8 .. 1.1e-7; the largest
    kernel / torch ratio of a case is 1.40 (forward)."""
    from dmayolo.functional import call, ptr, stream
    x, w, dz, p, OH, OW = _case(N, C, H, W, k, s, 100 * N + C + k + s + 13, torch.float32)
    xc, wc, dzc = x.cuda(), w.cuda(), dz.cuda()
    f64 = [F.conv2d(xc.double(), wc.double(), stride=s, padding=p, groups=C),
           torch.nn.grad.conv2d_input((N, C, H, W), wc.double(), dzc.double(), stride=s, padding=p, groups=C),
           torch.nn.grad.conv2d_weight(xc.double(), (C, 1, k, k), dzc.double(), stride=s, padding=p, groups=C)]
    t32 = [F.conv2d(xc, wc, stride=s, padding=p, groups=C),
           torch.nn.grad.conv2d_input((N, C, H, W), wc, dzc, stride=s, padding=p, groups=C),
           torch.nn.grad.conv2d_weight(xc, (C, 1, k, k), dzc, stride=s, padding=p, groups=C)]
    wd = _wop(w, torch.float32)
    _, xv = _slice(xc, Ct, c0)
    _, zv = _slice(dzc, Ct, c0)
    _, yv = _slice(torch.zeros_like(dzc), Ct, c0)
    _, dv = _slice(torch.zeros_like(xc), Ct, c0)
    call('dmy_dwconv_fwd', 0, ptr(xv), ptr(wd), None, ptr(yv), None, None, N, H, W, C, Ct, k, k, s, p, OH, OW, Ct,
         stream())
    call('dmy_dwconv_dgrad', 0, ptr(zv), ptr(wd), ptr(dv), 0, N, H, W, C, Ct, k, k, s, p, OH, OW, Ct, stream())
    P = call('dmy_dwconv_wgrad_rows', N * OH * OW, C)
    part, dw = torch.empty(P, k * k * C, device='cuda'), torch.empty(C, 1, k, k, device='cuda')
    call('dmy_dwconv_wgrad', 0, ptr(xv), ptr(zv), ptr(part), N, H, W, C, Ct, k, k, s, p, OH, OW, Ct, stream())
    call('dmy_dwconv_wgrad_finalize', ptr(part), P, C, k, k, ptr(dw), 0, stream())
    torch.cuda.synchronize()
    for name, got, a, b in zip(('fwd', 'dgrad', 'wgrad'), (yv, dv, dw), t32, f64):
        own, err = _rel(a, b), _rel(got, b)
        print(f'fp32 {name} {N, C, H, W} k{k} s{s}: torch {own:.2e} kernel {err:.2e}')
        assert err <= 4 * own, (name, err, own)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('k,s', GEOMS)
def test_dwconv_fwd_act_equals_two_passes(k, s, dtype):
    """dmy_dwconv_fwd_act == dmy_dwconv_fwd + dmy_bn_act_fwd to one storage rounding: bias, scale / shift, SiLU and a
    residual, input / output / residual all channel slices"""
    from dmayolo.functional import call, ptr, stream, ACT_SILU
    N, C, H, W, Ct, c0 = 3, 24, 19, 23, 48, 8
    dt = 1 if dtype == torch.bfloat16 else 0
    x, w, dz, p, OH, OW = _case(N, C, H, W, k, s, 5 + k + s, dtype)
    g = torch.Generator().manual_seed(9)
    bias, scale, shift = (torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda(),
                          torch.randn(C, generator=g).cuda())
    wd = _wop(w, dtype)
    _, xv = _slice(x.cuda(), Ct, c0)
    _, rv = _slice(dz.cuda(), Ct, c0)  # residual
    yb, yv = _slice(torch.zeros_like(dz), Ct, c0)
    _, zv = _slice(torch.zeros_like(dz), Ct, c0)
    _, y2 = _slice(torch.zeros_like(dz), Ct, c0)
    call('dmy_dwconv_fwd_act', dt, ptr(xv), ptr(wd), ptr(bias), ptr(yv), N, H, W, C, Ct, k, k, s, p, OH, OW, Ct,
         ptr(scale), ptr(shift), ACT_SILU, ptr(rv), Ct, stream())
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(bias), ptr(zv), None, None, N, H, W, C, Ct, k, k, s, p, OH, OW, Ct,
         stream())
    call('dmy_bn_act_fwd', dt, ptr(zv), Ct, ptr(scale), ptr(shift), ACT_SILU, ptr(rv), Ct, ptr(y2), Ct, N * OH * OW, C,
         stream())
    torch.cuda.synchronize()
    assert _others_untouched(yb, C, c0)
    a, b = yv.float(), y2.float()
    # one rounding of the stored value: an ulp of each intermediate both paths form -- u = z * scale + shift (a fused
    # or an unfused multiply-add, so one ulp of |z * scale| + |shift|, carried through SiLU whose slope is <= 1.1) and
    # the final act(u) + res (|act(u)| <= |u|) -- so where the terms cancel, the ulp is that of the terms, not the sum
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22
    u = (zv.float() * scale.view(1, -1, 1, 1)).abs() + shift.view(1, -1, 1, 1).abs()
    mag = 2.1 * u + rv.float().abs()
    assert bool(((a - b).abs() <= ulp * mag).all()), float(((a - b).abs() / mag.clamp_min(1e-30)).max())
    ref = F.silu((F.conv2d(x.float().cuda(), w.to(dtype).float().cuda(), stride=s, padding=p, groups=C) +
                  bias.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) + dz.float().cuda()
    assert _rel(a, ref) < 1e-2


def test_dwconv_unsupported_launches_nothing():
    """a geometry outside dmy_dwconv_ok: the query says 0, the entries return -1 (call() raises) and write nothing"""
    from dmayolo.functional import call, ptr, stream
    x = torch.zeros(1, 12, 8, 8, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)  # 12 % 8 != 0
    y = torch.full_like(x, float('nan'))
    w = torch.zeros(9, 12, dtype=torch.bfloat16, device='cuda')
    assert call('dmy_dwconv_ok', 1, ptr(x), ptr(w), ptr(y), 1, 8, 8, 12, 12, 12, 12, 3, 3, 1, 1, 8, 8, 12) == 0
    assert call('dmy_dwconv_ok', 1, ptr(x), ptr(w), ptr(y), 1, 8, 8, 16, 32, 2, 16, 3, 3, 1, 1, 8, 8, 16) == 0  # groups
    with pytest.raises(RuntimeError):
        call('dmy_dwconv_fwd', 1, ptr(x), ptr(w), None, ptr(y), None, None, 1, 8, 8, 12, 12, 3, 3, 1, 1, 8, 8, 12, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
