"""Kernel-level parity of dmy_layernorm_fwd / dmy_layernorm_bwd (csrc/swin.hip) and LayerNormFn against the fp64
restatement tests/eltwise_ref.py: every lanes-per-row form of the 16-byte-vector kernels (4 .. 64 lanes, with and
without idle lanes), the scalar kernels (fp32 C = 512 / 260, bf16 C = 260, C = 7, unaligned slices), strided x / dy / dx,
accumulate = 0 / 1, aligned and unaligned gamma / beta, the 1024-block cap with its grid-stride loop, and an input with a
large common offset.  Bounds as in tests/test_gpu_eltwise.py: per element, derived, printed before they are asserted."""
import pytest
import torch

import eltwise_ref as R
from test_gpu_eltwise import BF16, F32, DTYPES, FILL, _lib, check, dcode, gen_for, randn, slab, untouched

pytestmark = pytest.mark.gpu


def params(C, gen, aligned):
    """gamma around 1, beta around 0 on the device: 16-byte aligned, or a view one float into a larger tensor"""
    wc, bc = torch.randn(C, generator=gen) * 0.5 + 1, torch.randn(C, generator=gen)
    if aligned:
        return wc, bc, wc.cuda(), bc.cuda()
    w, b = torch.zeros(C + 1).cuda(), torch.zeros(C + 1).cuda()
    w[1:], b[1:] = wc.cuda(), bc.cuda()
    assert w[1:].data_ptr() % 16 == 4
    return wc, bc, w[1:], b[1:]


def run_fwd(xc, x, xps, wc, bc, w, b, eps, dtype, tag, check_y=True):
    call, ptr, stream = _lib()
    M, C = xc.shape
    y = torch.full((M, C), FILL, dtype=dtype, device='cuda')
    mean, rstd = torch.full((M,), FILL, device='cuda'), torch.full((M,), FILL, device='cuda')
    call('dmy_layernorm_fwd', dcode(dtype), ptr(x), xps, ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, C, eps, stream())
    yr, meanr, rstdr, ya, ma = R.layernorm_fwd(xc.double(), wc.double(), bc.double(), eps)
    check(f'ln_mean{tag}', mean, meanr, ma, C, F32)                 # C - 1 additions and the division
    check(f'ln_rstd{tag}', rstd, rstdr, 0 * rstdr, 0, F32, trans=True)
    if check_y:
        # (x - mean) rstd w + b: the mean's own bound, scaled by |rstd w|, on top of the elementwise and rsqrt bounds
        check(f'ln_y{tag}', y, yr, ya, 4, dtype, trans=True, extra=(rstdr[:, None] * wc.double()).abs() * (C * R.U32 * ma)[:, None])
    return mean, rstd


def run_bwd(xc, x, xps, dyc, wc, w, mean, rstd, dtype, Ct, off, tag):
    """both accumulate modes into a strided dx; -> the partial rows of the last run"""
    call, ptr, stream = _lib()
    M, C = xc.shape
    gbuf, dy = slab(dyc, Ct, off)
    P = call('dmy_layernorm_bwd_blocks', M)
    dxr, dwr, dbr, adx, aa1, aa2, adw, adb = R.layernorm_bwd(xc.double(), dyc.double(), wc.double(), mean.double().cpu(),
                                                             rstd.double().cpu())
    pre = randn((M, C), gen_for(M, C, 9), dtype)
    for acc in (0, 1):
        dbuf, dx = slab(pre, Ct, off)
        pdw, pdb = torch.full((P, C), FILL, device='cuda'), torch.full((P, C), FILL, device='cuda')
        call('dmy_layernorm_bwd', dcode(dtype), ptr(x), xps, ptr(dy), Ct, ptr(w), ptr(mean), ptr(rstd), ptr(dx), Ct, acc,
             M, C, ptr(pdw), ptr(pdb), stream())
        base = pre.double() * acc
        # the two row means (C terms each) inside dx follow the sum bound, the rest is elementwise
        check(f'ln_dx_acc{acc}{tag}', dx, dxr + base, adx + base.abs(), 4, dtype, extra=C * R.U32 * (aa1 + aa2))
        assert untouched(dbuf, off, C)
        # the P partial rows, summed in row order: M terms per channel (each a product of three roundings for dw)
        check(f'ln_dw{tag}', pdw.double().sum(0), dwr, adw, M + 3, F32)
        check(f'ln_db{tag}', pdb.double().sum(0), dbr, adb, M, F32)
    assert untouched(gbuf, off, C)
    return pdw, pdb


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('eps', [1e-5, 1e-6])
@pytest.mark.parametrize('M', [1, 37, 67])
@pytest.mark.parametrize('C', [32, 24, 96, 512, 260, 7])
def test_layernorm(C, M, eps, dtype):
    gen = gen_for(C, M)
    Ct, off = C + 8, 8                       # x, dy and dx are channel slices of wider buffers
    xc = (torch.randn((M, C), generator=gen) * 0.7 + 0.3).to(dtype)
    dyc = randn((M, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    for aligned in (True, False):
        wc, bc, w, b = params(C, gen, aligned)
        tag = '' if aligned else '_unaligned'
        mean, rstd = run_fwd(xc, x, Ct, wc, bc, w, b, eps, dtype, tag)
        run_bwd(xc, x, Ct, dyc, wc, w, mean, rstd, dtype, Ct, off, tag)
    assert untouched(xbuf, off, C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lanes', [4, 8, 16, 32, 64, 128])
def test_layernorm_every_lane_count(lanes, dtype):
    """C = lanes x one 16-byte vector, M = 7 rows: each lane count the vector kernels are built for (4 .. 64) in each
    storage type, and 128 lanes, which they refuse, so the scalar kernels run"""
    C, M, eps = lanes * (8 if dtype == BF16 else 4), 7, 1e-5
    gen = gen_for(C, M, lanes)
    Ct, off = C + 8, 8
    xc = (torch.randn((M, C), generator=gen) * 0.7 + 0.3).to(dtype)
    dyc = randn((M, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    wc, bc, w, b = params(C, gen, True)
    mean, rstd = run_fwd(xc, x, Ct, wc, bc, w, b, eps, dtype, f'_lanes{lanes}')
    run_bwd(xc, x, Ct, dyc, wc, w, mean, rstd, dtype, Ct, off, f'_lanes{lanes}')
    assert untouched(xbuf, off, C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('off', [8, 3])
def test_layernorm_many_rows(off, dtype):
    """M = 70 000 rows of 32 channels: the backward's 1024-block cap and both kernels' grid-stride loops; a slice at a
    vector-multiple offset runs the vector kernels, one at offset 3 the scalar ones, whose blocks take
    ceil(M / 1024) = 69 rows each, so the last 9 of the 1024 own no row and their partials are exactly zero"""
    M, C, Ct = 70000, 32, 48
    gen = gen_for(off)
    xc = (torch.randn((M, C), generator=gen) * 0.7 + 0.3).to(dtype)
    dyc = randn((M, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    wc, bc, w, b = params(C, gen, True)
    mean, rstd = run_fwd(xc, x, Ct, wc, bc, w, b, 1e-5, dtype, '_70k')
    pdw, pdb = run_bwd(xc, x, Ct, dyc, wc, w, mean, rstd, dtype, Ct, off, '_70k')
    P = pdw.shape[0]
    assert P == 1024
    if off == 3:
        rpb = -(-M // P)
        first_empty = -(-M // rpb)
        assert first_empty == 1015
        assert bool((pdw[first_empty:] == 0).all()) and bool((pdb[first_empty:] == 0).all())
        assert bool((pdb[:first_empty].abs().sum(1) > 0).all())


@pytest.mark.parametrize('C', [32, 260])
def test_layernorm_large_common_offset(C):
    """rows with mean 50 and standard deviation 0.1 (fp32): the variance is taken around the mean, so rstd (about 10)
    still matches the fp64 value within the rsqrt bound; E[x^2] - mean^2 in fp32 would be off by several percent"""
    M, eps = 37, 1e-5
    gen = gen_for(C, 50)
    xc = (torch.randn((M, C), generator=gen) * 0.1 + 50).float()
    x = xc.cuda()
    wc, bc, w, b = params(C, gen, True)
    run_fwd(xc, x, C, wc, bc, w, b, eps, F32, '_offset50', check_y=False)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [24, 260])
def test_layernorm_fn(C, dtype):
    """the autograd wrapper: pixel strides, the gradient sink and the fold of the partial rows (dmy_reduce_rows)"""
    from dmayolo.functional import LayerNormFn, GradSink
    N, H, W, eps = 2, 5, 7, 1e-6
    M = N * H * W
    gen = gen_for(C, 77)
    xc = (torch.randn((N, H, W, C), generator=gen) * 0.7 + 0.3).to(dtype)
    dyc, pre = randn((N, H, W, C), gen, dtype), randn((N, H, W, C), gen, dtype)
    xbuf, xs = slab(xc, C + 8, 8)
    x = xs.permute(0, 3, 1, 2).requires_grad_(True)
    wc, bc = torch.randn(C, generator=gen) * 0.5 + 1, torch.randn(C, generator=gen)
    w, b = wc.cuda().requires_grad_(True), bc.cuda().requires_grad_(True)
    sink = GradSink(2)
    y = LayerNormFn.apply(x, w, b, eps, sink)
    x2, dy2 = xc.double().view(M, C), dyc.double().view(M, C)
    yr, meanr, rstdr, ya, ma = R.layernorm_fwd(x2, wc.double(), bc.double(), eps)
    prop = (rstdr[:, None] * wc.double()).abs() * (C * R.U32 * ma)[:, None]
    check('LayerNormFn_y', y.permute(0, 2, 3, 1), yr.view(N, H, W, C), ya.view(N, H, W, C), 4, dtype, trans=True,
          extra=prop.view(N, H, W, C))
    assert sink.passthrough(pre.cuda().permute(0, 3, 1, 2)) is None
    gb, gs = slab(dyc, C + 8, 8)
    y.backward(gs.permute(0, 3, 1, 2))
    # against the fp64 statistics: the saved fp32 mean / rstd are within their own bounds of these (checked above), and
    # dx, dw, db are smooth in them, so the rsqrt tolerance covers the difference
    dxr, dwr, dbr, adx, aa1, aa2, adw, adb = R.layernorm_bwd(x2, dy2, wc.double(), meanr, rstdr)
    base = pre.double().view(M, C)
    check('LayerNormFn_dx', x.grad.permute(0, 2, 3, 1).reshape(M, C), dxr + base, adx + base.abs(), 4, dtype, trans=True,
          extra=C * R.U32 * (aa1 + aa2) + prop)
    check('LayerNormFn_dw', w.grad, dwr, adw, M + 3, F32, trans=True)
    check('LayerNormFn_db', b.grad, dbr, adb, M, F32)
