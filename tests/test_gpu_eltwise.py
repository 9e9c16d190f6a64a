"""Kernel-level parity of the gating / attention / layout kernels of csrc/eltwise.hip against the fp64 restatement
tests/eltwise_ref.py (itself checked on the CPU by tests/test_eltwise_ref.py):

  dmy_avgpool_fwd/bwd, dmy_resize_fwd/bwd, dmy_scgate_fwd/bwd, dmy_ca_pool_fwd/bwd, dmy_ca_apply_fwd/bwd,
  dmy_halves_sigmoid, dmy_cbam_in_fwd/bwd, dmy_pixscale, dmy_nchw_to_nhwc, dmy_nhwc_to_nchw_f32, dmy_pointwise, dmy_cast
  and the autograd wrappers AvgPoolFn, ResizeFn, SCGateFn, CAPoolFn, CAApplyFn, HalvesSigmoidFn, CBAMInFn, PixScaleFn.

Every entry point runs in its 16-byte-vector and its scalar form (channel counts that are / are not a vector multiple,
slices of a wider buffer at an aligned / unaligned channel offset) and with accumulate = 0 / 1 where it has the flag.
The bounds are per element and derived (eltwise_ref.bound): pure data movement and maxima are bit-exact, fp32 arithmetic
is n * 2^-24 * sum|term|, bf16 storage adds 2^-8 |ref|, and what passes through sigmoid / erf adds the project's fp32
elementwise tolerance (rtol = atol = 1e-5); the measured errors of those are in DESIGN.md.  Every `check` prints its
worst error before it asserts.
"""
import pytest
import torch

import eltwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [BF16, F32]
FILL = 7.0   # what the channels of a wider buffer outside the slice hold, before and after


def _lib():
    from dmayolo.functional import call, ptr, stream
    return call, ptr, stream


def dcode(dtype):
    return 1 if dtype == BF16 else 0


def gen_for(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k * 8) if isinstance(k, float) else k for k in key))) % (2 ** 31))


def randn(shape, gen, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


def grid(shape, gen, lo, hi, step, dtype):
    """integers lo..hi times step: exact in bf16 and fp32 for the small ranges used here"""
    return (torch.randint(lo, hi + 1, shape, generator=gen).float() * step).to(dtype)


def slab(t, Ct, off):
    """the CPU tensor t [..., C] as the channel slice [off, off + C) of a device buffer [..., Ct] -> (buffer, view)"""
    C = t.shape[-1]
    buf = torch.full((*t.shape[:-1], Ct), FILL, dtype=t.dtype)
    buf[..., off:off + C] = t
    buf = buf.cuda()
    return buf, buf[..., off:off + C]


def untouched(buf, off, C):
    return bool((buf[..., :off] == FILL).all()) and bool((buf[..., off + C:] == FILL).all())


def check(name, out, ref, abssum, n, dtype, trans=False, ref2=None, extra=0.0):
    """|out - ref| <= eltwise_ref.bound (+ extra, a derived allowance the caller explains) elementwise; ref2: a second
    admissible reference, out may lie between the two"""
    o = out.detach().double().cpu().reshape(ref.shape)
    lo, hi = (ref, ref) if ref2 is None else (torch.minimum(ref, ref2), torch.maximum(ref, ref2))
    err = torch.clamp(torch.maximum(lo - o, o - hi), min=0)
    err = torch.where(torch.isfinite(o), err, torch.full_like(err, float('inf')))
    b = R.bound(ref, abssum, n, dtype, trans) + extra
    ratio = float((err / b.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'MEASURE {name} {str(dtype)[6:]} trans={int(trans)} max_err={float(err.max()):.3e} err/bound={ratio:.4f}')
    bad = err > b
    assert not bool(bad.any()), f'{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/bound {ratio:.3f}'


def equal(a, ref):
    return torch.equal(a.detach().double().cpu().reshape(ref.shape), ref)


# layouts (C, Ct, off): dense vector in both types / vector in fp32 only / scalar in both, then a 16-channel slice of a
# 40-channel buffer at a vector-multiple offset (strided vector form) and at an offset that is not (scalar form)
LAYOUTS = [(16, 16, 0), (12, 12, 0), (6, 6, 0), (16, 40, 8), (16, 40, 3)]


# ---------------------------------------------------------------- A. avg-pool
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,Ct,off', LAYOUTS)
@pytest.mark.parametrize('N,H,W', [(2, 9, 14), (1, 17, 23), (2, 8, 8)])
@pytest.mark.parametrize('r', [2, 4])
def test_avgpool(r, N, H, W, C, Ct, off, dtype):
    call, ptr, stream = _lib()
    gen = gen_for(r, H, C, off)
    dt, OH, OW = dcode(dtype), H // r, W // r
    xc = randn((N, H, W, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    y = torch.full((N, OH, OW, C), FILL, dtype=dtype, device='cuda')
    call('dmy_avgpool_fwd', dt, ptr(x), Ct, ptr(y), N, H, W, C, r, stream())
    yr, ya = R.avgpool_fwd(xc.double(), r)
    check('avgpool_fwd', y, yr, ya, r * r, dtype)   # r * r - 1 additions and the scaling

    dyc = randn((N, OH, OW, C), gen, dtype)
    dy = dyc.cuda()
    dxr, dxa = R.avgpool_bwd(dyc.double(), H, W, r)
    pre = randn((N, H, W, C), gen, dtype)
    for acc in (0, 1):
        dbuf, dx = slab(pre, Ct, off)
        call('dmy_avgpool_bwd', dt, ptr(dy), ptr(dx), Ct, acc, N, H, W, C, r, stream())
        assert untouched(dbuf, off, C)
        base = pre.double() * acc
        check(f'avgpool_bwd_acc{acc}', dx, dxr + base, dxa + base.abs(), 4, dtype)
        # floor mode: the trailing rows / columns get exactly zero gradient (the prefilled value survives bit-exact)
        border = torch.ones(H, W, dtype=torch.bool)
        border[:OH * r, :OW * r] = False
        assert torch.equal(dx.cpu()[:, border], (pre * acc)[:, border] if acc else torch.zeros_like(pre)[:, border])
    torch.cuda.synchronize()


# ---------------------------------------------------------------- B. nearest resize
RESIZES = [((5, 7), (10, 14)), ((5, 7), (5, 7)), ((5, 7), (13, 20)), ((4, 5), (17, 23)), ((13, 20), (5, 7))]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [16, 6])
@pytest.mark.parametrize('src,dst', RESIZES)
def test_resize(src, dst, C, dtype):
    import torch.nn.functional as F
    call, ptr, stream = _lib()
    (IH, IW), (OH, OW), N, dt = src, dst, 2, dcode(dtype)
    gen = gen_for(IH, OH, C)
    Ct, off = C + 8, 8            # the output is a channel slice of a concat buffer: vector form at C = 16, scalar at 6
    xc = randn((N, IH, IW, C), gen, dtype)
    x = xc.cuda()
    ybuf, y = slab(torch.full((N, OH, OW, C), FILL, dtype=dtype), Ct, off)
    call('dmy_resize_fwd', dt, ptr(x), C, ptr(y), Ct, 1.0, N, IH, IW, OH, OW, C, stream())
    want = F.interpolate(xc.float().permute(0, 3, 1, 2), size=dst, mode='nearest').permute(0, 2, 3, 1).double()
    assert equal(y, want) and untouched(ybuf, off, C)          # the index map is ATen's; pure data movement
    assert torch.equal(R.resize_fwd(xc.double(), OH, OW)[0], want)

    dyc = randn((N, OH, OW, C), gen, dtype)
    dbuf, dy = slab(dyc, Ct, off)                                  # dy strided
    dx = torch.full((N, IH, IW, C), FILL, dtype=dtype, device='cuda')
    call('dmy_resize_bwd', dt, ptr(dy), Ct, ptr(dx), C, N, IH, IW, OH, OW, C, stream())
    dxr, dxa = R.resize_bwd(dyc.double(), IH, IW)
    check('resize_bwd', dx, dxr, dxa, max(4, R.resize_max_preimage(IH, IW, OH, OW)), dtype)
    if OH < IH:  # a window edge: input pixels with no preimage get exactly zero
        assert bool((dx.cpu().double()[dxa == 0] == 0).all()) and bool((dxa == 0).any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_resize_scaled(dtype):
    call, ptr, stream = _lib()
    N, IH, IW, OH, OW, C = 2, 5, 7, 13, 20, 16
    xc = randn((N, IH, IW, C), gen_for(5), dtype)
    x = xc.cuda()
    y = torch.empty((N, OH, OW, C), dtype=dtype, device='cuda')
    call('dmy_resize_fwd', dcode(dtype), ptr(x), C, ptr(y), C, 0.5, N, IH, IW, OH, OW, C, stream())
    yr, ya = R.resize_fwd(xc.double(), OH, OW, 0.5)
    check('resize_fwd_half', y, yr, ya, 4, dtype)


# ---------------------------------------------------------------- C. SCConv gate
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [16, 6])
@pytest.mark.parametrize('H,W,GH,GW', [(16, 16, 4, 4), (17, 23, 4, 5), (9, 6, 2, 1)])
def test_scgate(H, W, GH, GW, C, dtype):
    call, ptr, stream = _lib()
    N, dt, Ct, off = 2, dcode(dtype), C + 8, 8
    gen = gen_for(H, GW, C)
    # x and g on a grid of 1/16 in [-4, 4]: x + g is exact in every type (its storage rounding is the identity) and
    # the logit stays in [-8, 8]
    xc, gc = grid((N, H, W, C), gen, -64, 64, 1 / 16, dtype), grid((N, GH, GW, C), gen, -64, 64, 1 / 16, dtype)
    uc, dc = randn((N, H, W, C), gen, dtype), randn((N, H, W, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    u3, g, dout = uc.cuda(), gc.cuda(), dc.cuda()
    out = torch.empty((N, H, W, C), dtype=dtype, device='cuda')
    call('dmy_scgate_fwd', dt, ptr(x), Ct, ptr(u3), ptr(g), ptr(out), N, H, W, C, GH, GW, stream())
    ref, s, oa = R.scgate_fwd(xc.double(), uc.double(), gc.double(), dtype)
    if dtype == BF16:
        # the sigmoid is rounded to bf16 before the product (documented): a kernel sigmoid within 1e-5 (1 + s) of the
        # fp64 one may round to the neighbouring bf16 value, so the product may lie between the two roundings
        d = R.TRANS * (1 + s)
        a, b = uc.double() * R.rnd(s - d, dtype), uc.double() * R.rnd(s + d, dtype)
        check('scgate_fwd', out, a, oa, 4, dtype, ref2=b)
    else:
        check('scgate_fwd', out, ref, oa, 4, dtype, trans=True)

    du3r, dprer, a3, ap = R.scgate_bwd(xc.double(), uc.double(), gc.double(), dc.double(), dtype)
    pre = randn((N, H, W, C), gen, dtype)
    for acc in (0, 1):
        du3 = torch.empty((N, H, W, C), dtype=dtype, device='cuda')
        pbuf, dpre = slab(pre, Ct, off)
        call('dmy_scgate_bwd', dt, ptr(x), Ct, ptr(u3), ptr(g), ptr(dout), ptr(du3), ptr(dpre), Ct, acc, N, H, W, C,
             GH, GW, stream())
        base = pre.double() * acc
        check('scgate_bwd_du3', du3, du3r, a3, 4, dtype, trans=True)
        check(f'scgate_bwd_dpre_acc{acc}', dpre, dprer + base, ap + base.abs(), 4, dtype, trans=True)
        assert untouched(pbuf, off, C)
    assert untouched(xbuf, off, C)


# ---------------------------------------------------------------- D. CoorAttention
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,H,W,C', [(2, 5, 9, 6), (1, 12, 3, 16), (3, 1, 7, 8)])
def test_coorattention(N, H, W, C, dtype):
    call, ptr, stream = _lib()
    dt, Ct, off = dcode(dtype), C + 8, 8
    gen = gen_for(N, H, W, C)
    xc = randn((N, H, W, C), gen, dtype)
    xbuf, x = slab(xc, Ct, off)
    y = torch.empty((N, H + W, C), dtype=dtype, device='cuda')
    call('dmy_ca_pool_fwd', dt, ptr(x), Ct, ptr(y), N, H, W, C, stream())
    yr, ya = R.ca_pool_fwd(xc.double())
    # rows: W terms, columns: H terms (n - 1 additions and the division); H != W, so a swapped divisor shows
    check('ca_pool_rows', y[:, :H], yr[:, :H], ya[:, :H], W, dtype)
    check('ca_pool_cols', y[:, H:], yr[:, H:], ya[:, H:], H, dtype)

    dyc = randn((N, H + W, C), gen, dtype)
    dy = dyc.cuda()
    dxr, dxa = R.ca_pool_bwd(dyc.double(), H, W)
    pre = randn((N, H, W, C), gen, dtype)
    for acc in (0, 1):
        dbuf, dx = slab(pre, Ct, off)
        call('dmy_ca_pool_bwd', dt, ptr(dy), ptr(dx), Ct, acc, N, H, W, C, stream())
        base = pre.double() * acc
        check(f'ca_pool_bwd_acc{acc}', dx, dxr + base, dxa + base.abs(), 4, dtype)
        assert untouched(dbuf, off, C)

    lhc = (torch.rand((N, H + W, C), generator=gen) * 16 - 8).to(dtype)   # logits in [-8, 8]
    lwc = (torch.rand((N, H + W, C), generator=gen) * 16 - 8).to(dtype)
    lh, lw = lhc.cuda(), lwc.cuda()
    obuf, out = slab(torch.full((N, H, W, C), FILL, dtype=dtype), Ct, off)
    call('dmy_ca_apply_fwd', dt, ptr(x), Ct, ptr(lh), ptr(lw), ptr(out), Ct, N, H, W, C, stream())
    outr, outa = R.ca_apply_fwd(xc.double(), lhc.double(), lwc.double())
    check('ca_apply_fwd', out, outr, outa, 4, dtype, trans=True)
    assert untouched(obuf, off, C)

    doc = randn((N, H, W, C), gen, dtype)
    gbuf, dout = slab(doc, Ct, off)
    dbuf, dx = slab(torch.full((N, H, W, C), FILL, dtype=dtype), Ct, off)
    dlh = torch.full((N, H + W, C), FILL, dtype=dtype, device='cuda')
    dlw = torch.full((N, H + W, C), FILL, dtype=dtype, device='cuda')
    call('dmy_ca_apply_bwd', dt, ptr(x), Ct, ptr(lh), ptr(lw), ptr(dout), Ct, ptr(dx), Ct, ptr(dlh), ptr(dlw), N, H, W,
         C, stream())
    dxr, dlhr, dlwr, dxa, alh, alw = R.ca_apply_bwd(xc.double(), lhc.double(), lwc.double(), doc.double())
    check('ca_apply_bwd_dx', dx, dxr, dxa, 4, dtype, trans=True)
    # a row sum of W (H) terms, each a product of four factors, and the two closing factors: n = terms + 5 roundings
    check('ca_apply_bwd_dlh', dlh[:, :H], dlhr[:, :H], alh[:, :H], W + 5, dtype, trans=True)
    check('ca_apply_bwd_dlw', dlw[:, H:], dlwr[:, H:], alw[:, H:], H + 5, dtype, trans=True)
    assert bool((dlh[:, H:] == 0).all()) and bool((dlw[:, :H] == 0).all())   # exactly zero
    assert untouched(dbuf, off, C) and untouched(xbuf, off, C) and untouched(gbuf, off, C)


# ---------------------------------------------------------------- E. CBAM
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [16, 6, 520])
@pytest.mark.parametrize('N', [1, 3])
def test_halves_sigmoid(N, C, dtype):
    call, ptr, stream = _lib()
    gen = gen_for(N, C)
    zc = grid((2 * N, C), gen, -64, 64, 1 / 16, dtype)   # the sum of the halves is exact and in [-8, 8]
    dcc = randn((N, C), gen, dtype)
    z, dca = zc.cuda(), dcc.cuda()
    ca = torch.empty((N, C), dtype=dtype, device='cuda')
    call('dmy_halves_sigmoid', dcode(dtype), ptr(z), N, C, ptr(ca), None, None, stream())
    car = R.halves_sigmoid_fwd(zc.double(), dtype)
    check('halves_sigmoid_fwd', ca, car, car, 4, dtype, trans=True)
    dz = torch.empty((2 * N, C), dtype=dtype, device='cuda')
    call('dmy_halves_sigmoid', dcode(dtype), ptr(z), N, C, None, ptr(dca), ptr(dz), stream())
    dzr = R.halves_sigmoid_bwd(zc.double(), dcc.double(), dtype)
    check('halves_sigmoid_bwd', dz, dzr, dzr.abs(), 4, dtype, trans=True)
    assert torch.equal(dz[:N], dz[N:])   # both halves receive the same gradient bit for bit


# C: 16 idle lanes / 6 scalar / 70 scalar, two trips of the 64-lane channel loop / 520 bf16 vector with two trips;
# 260 (fp32 only) vector with 65 lanes' worth.  HW: below, at and above one 64-pixel wave chunk, the last one partial
@pytest.mark.parametrize('dtype,C', [(d, c) for d in DTYPES for c in (16, 6, 70, 520)] + [(F32, 260)])
@pytest.mark.parametrize('HW', [7, 64, 150])
@pytest.mark.parametrize('N', [1, 3])
def test_cbam(N, HW, C, dtype):
    call, ptr, stream = _lib()
    dt, Ct, off = dcode(dtype), C + 8, 8
    gen = gen_for(N, HW, C)
    # x on multiples of 1/4 in [-2, 2], ca on multiples of 1/8 in (0, 1]: x * ca is exact in bf16, fp32 and fp64, so
    # its storage rounding is the identity and ties of the channel maximum are real ties
    xc = grid((N, HW, C), gen, -8, 8, 1 / 4, dtype)
    cac = grid((N, C), gen, 1, 8, 1 / 8, dtype)
    xc[:, 0, :], cac[:, 2], cac[:, 5] = 2.0, 1.0, 1.0     # pixel 0: channels 2 and 5 (at least) share the maximum 2.0
    xbuf, x = slab(xc, Ct, off)
    ca = cac.cuda()
    out1 = torch.empty((N, HW, C), dtype=dtype, device='cuda')
    s2 = torch.empty((N, HW, 2), dtype=dtype, device='cuda')
    am = torch.empty((N, HW), dtype=torch.int32, device='cuda')
    call('dmy_cbam_in_fwd', dt, ptr(x), Ct, ptr(ca), N, HW, C, ptr(out1), ptr(s2), ptr(am), stream())
    o1r, meanr, mxr, amr, ma = R.cbam_in_fwd(xc.double(), cac.double(), dtype)
    assert equal(out1, o1r) and equal(s2[..., 1], mxr)
    assert torch.equal(am.cpu().long(), amr)                     # the first channel wins a tie
    assert int((o1r == mxr[..., None]).sum(-1).max()) > 1 and int(amr[:, 0].max()) <= 2   # ... and there are ties
    check('cbam_mean', s2[..., 0], meanr, ma, C, dtype)

    d1c, ds2c = randn((N, HW, C), gen, dtype), randn((N, HW, 2), gen, dtype)
    gbuf, dout1 = slab(d1c, Ct, off)
    ds2 = ds2c.cuda()
    dxr, dcar, dxa, dcaa = R.cbam_in_bwd(xc.double(), cac.double(), d1c.double(), ds2c.double(), amr)
    pre = randn((N, HW, C), gen, dtype)
    nws = call('dmy_cbam_in_bwd_ws_elems', N, HW, C)
    runs = []
    for acc in (0, 1, 1):
        dbuf, dx = slab(pre, Ct, off)
        dca = torch.full((N, C), FILL, device='cuda')
        ws = torch.full((nws,), FILL, device='cuda')
        call('dmy_cbam_in_bwd', dt, ptr(x), Ct, ptr(ca), ptr(dout1), Ct, ptr(ds2), ptr(am), N, HW, C, ptr(dx), Ct, acc,
             ptr(dca), ptr(ws), stream())
        base = pre.double() * acc
        check(f'cbam_dx_acc{acc}', dx, dxr + base, dxa + base.abs(), 4, dtype)
        # HW terms, each (dout1 + dmean / C + dmax) * x: three roundings and the product on top of the HW - 1 additions
        check('cbam_dca', dca, dcar, dcaa, HW + 4, F32)
        assert untouched(dbuf, off, C)
        runs.append(dca.clone())
    assert torch.equal(runs[1], runs[2]) and torch.equal(runs[0], runs[1])   # run-to-run bit-identical

    # spatial attention's product: sa one value per pixel, read with stride 1 or 8
    sps = 1 if N == 1 else 8
    sac = torch.rand((N, HW), generator=gen).to(dtype)
    sabuf, sa = slab(sac[..., None], sps, 0)
    obuf, out = slab(torch.full((N, HW, C), FILL, dtype=dtype), Ct, off)
    call('dmy_pixscale', dt, ptr(out1), ptr(sa), sps, N, HW, C, ptr(out), Ct, None, 0, None, None, stream())
    o1 = out1.cpu().double()
    outr, outa = R.pixscale_fwd(o1, sac.double())
    check('pixscale_fwd', out, outr, outa, 4, dtype)
    assert untouched(obuf, off, C)
    g1 = torch.empty((N, HW, C), dtype=dtype, device='cuda')
    dsa = torch.empty((N, HW), dtype=dtype, device='cuda')
    call('dmy_pixscale', dt, ptr(out1), ptr(sa), sps, N, HW, C, None, 0, ptr(dout1), Ct, ptr(g1), ptr(dsa), stream())
    g1r, dsar, g1a, dsaa = R.pixscale_bwd(o1, sac.double(), d1c.double())
    check('pixscale_dout1', g1, g1r, g1a, 4, dtype)
    check('pixscale_dsa', dsa, dsar, dsaa, C + 1, dtype)   # C products summed
    assert untouched(xbuf, off, C) and untouched(gbuf, off, C)


# ---------------------------------------------------------------- G. layout and pointwise
@pytest.mark.parametrize('dtype,Cp', [(BF16, 8), (F32, 4), (F32, 8)])
@pytest.mark.parametrize('src', [torch.uint8, F32])
@pytest.mark.parametrize('scale', [1.0, 1.0 / 255.0])
def test_nchw_to_nhwc(dtype, Cp, src, scale):
    call, ptr, stream = _lib()
    N, C, H, W = 2, 3, 19, 31   # H * W = 589: not a multiple of 256, more than one block
    gen = gen_for(Cp, scale)
    xs = torch.randint(0, 256, (N, C, H, W), generator=gen, dtype=torch.uint8)
    if src == F32:
        xs = xs.float() / 4 - 30     # exact in bf16: scale 1 is pure data movement in both types
    x = xs.cuda()
    y = torch.full((N, H, W, Cp), FILL, dtype=dtype, device='cuda')
    call('dmy_nchw_to_nhwc', dcode(dtype), 0 if src == torch.uint8 else 1, ptr(x), ptr(y), N, C, H, W, Cp, scale, stream())
    ref = R.nchw_to_nhwc(xs, Cp, scale)
    assert bool((y[..., C:] == 0).all())                      # the padding channels are exactly zero
    if scale == 1.0:
        assert equal(y, R.rnd(ref, dtype))                       # uint8 0..255 rounds once to bf16, as torch does
    else:
        check('nchw_to_nhwc', y, ref, ref.abs(), 4, dtype)


@pytest.mark.parametrize('dtype,Cp', [(BF16, 12), (BF16, 4), (F32, 6), (F32, 3)])
def test_nchw_to_nhwc_rejects_partial_vectors(dtype, Cp):
    """the contract: the pixel stride Cp is a whole number of 16-byte vectors (functional.vec_pad gives every caller
    one) and the output is 16-byte aligned; anything else is refused before a launch"""
    call, ptr, stream = _lib()
    x = torch.zeros((1, 3, 4, 4), device='cuda')
    y = torch.full((1, 4, 4, 16), FILL, dtype=dtype, device='cuda')
    with pytest.raises(RuntimeError, match='dmy_nchw_to_nhwc failed with hipError 1'):
        call('dmy_nchw_to_nhwc', dcode(dtype), 1, ptr(x), ptr(y), 1, 3, 4, 4, Cp, 1.0, stream())
    with pytest.raises(RuntimeError, match='dmy_nchw_to_nhwc failed with hipError 1'):   # unaligned output
        call('dmy_nchw_to_nhwc', dcode(dtype), 1, ptr(x), ptr(y.view(-1)[1:]), 1, 3, 4, 4, 8, 1.0, stream())
    torch.cuda.synchronize()
    assert bool((y == FILL).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_nhwc_to_nchw_f32(dtype):
    call, ptr, stream = _lib()
    N, C, H, W, Ct, off = 2, 3, 19, 31, 8, 2
    xc = randn((N, H, W, C), gen_for(3), dtype)
    xbuf, x = slab(xc, Ct, off)
    y = torch.empty((N, C, H, W), device='cuda')
    call('dmy_nhwc_to_nchw_f32', dcode(dtype), ptr(x), Ct, ptr(y), N, C, H, W, stream())
    assert equal(y, R.nhwc_to_nchw(xc))


POINTWISE_N = 1000   # not a multiple of 256


def _pw(dtype, op, act, a, b, alpha):
    call, ptr, stream = _lib()
    y = torch.empty_like(a)
    call('dmy_pointwise', dcode(dtype), op, act, ptr(a), ptr(b), ptr(y), a.numel(), alpha, stream())
    return y


@pytest.mark.parametrize('dtype', DTYPES)
def test_pointwise_linear(dtype):
    gen = gen_for(11)
    ac, bc = grid((POINTWISE_N,), gen, -40, 40, 1 / 4, dtype), grid((POINTWISE_N,), gen, -40, 40, 1 / 4, dtype)
    a, b = ac.cuda(), bc.cuda()
    assert equal(_pw(dtype, 0, 0, a, b, 1.0), ac.double() + bc.double())     # grid values: the sum is exact
    ac, bc = randn((POINTWISE_N,), gen, dtype), randn((POINTWISE_N,), gen, dtype)
    a, b = ac.cuda(), bc.cuda()
    alpha = float(torch.tensor(0.3, dtype=F32))
    for op in (0, 3, 4):
        ref, ra = R.pointwise(op, 0, ac.double(), bc.double(), alpha)
        check(f'pointwise_op{op}', _pw(dtype, op, 0, a, b, alpha), ref, ra, 4, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', range(7))
def test_pointwise_act(act, dtype):
    gen = gen_for(act)
    kinks = torch.tensor([-3.0, 3.0, 0.0, -0.0, -8.0, 8.0, -3.015625, 3.015625, 2.984375])
    ac = torch.cat([kinks, torch.rand(POINTWISE_N - kinks.numel(), generator=gen) * 16 - 8]).to(dtype)
    bc = randn((POINTWISE_N,), gen, dtype)
    a, b = ac.cuda(), bc.cuda()
    trans = act in R.ACT_TRANS
    ref, ra = R.pointwise(1, act, ac.double(), None, 0.0)
    check(f'act{act}_fwd', _pw(dtype, 1, act, a, b, 0.0), ref, ra, 4, dtype, trans=trans)
    ref, ra = R.pointwise(2, act, ac.double(), bc.double(), 0.0)
    check(f'act{act}_grad', _pw(dtype, 2, act, a, b, 0.0), ref, ra, 4, dtype, trans=trans)


@pytest.mark.parametrize('sk,dk', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_cast(sk, dk):
    call, ptr, stream = _lib()
    kinds = {0: F32, 1: BF16}
    xc = randn((POINTWISE_N,), gen_for(sk, dk), kinds[sk])
    x = xc.cuda()
    for scale in (1.0, 0.5, 1.0 / 255.0):
        y = torch.empty(POINTWISE_N, dtype=kinds[dk], device='cuda')
        call('dmy_cast', sk, dk, ptr(x), ptr(y), POINTWISE_N, scale, stream())
        ref = xc.double() * float(torch.tensor(scale, dtype=F32))
        if scale != 1.0 / 255.0:   # exact product: one rounding to the destination, torch's own
            assert equal(y, R.rnd(ref, kinds[dk]))
        else:
            check('cast_scaled', y, ref, ref.abs(), 4, kinds[dk])


# ---------------------------------------------------------------- the autograd wrappers (Python glue: strides, sinks)
def cl(t):
    """NHWC CPU tensor -> logical NCHW channels_last device tensor"""
    return t.cuda().permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_avgpool_fn_with_sink(dtype):
    from dmayolo.functional import AvgPoolFn, GradSink
    N, H, W, C, r = 2, 9, 14, 16, 2
    gen = gen_for(1)
    xc, dyc, pre = randn((N, H, W, C), gen, dtype), randn((N, 4, 7, C), gen, dtype), randn((N, H, W, C), gen, dtype)
    xbuf, xs = slab(xc, 24, 8)                       # a channel slice: the pixel stride reaches the kernel
    x = xs.permute(0, 3, 1, 2).requires_grad_(True)
    sink = GradSink(2)
    y = AvgPoolFn.apply(x, r, sink)
    yr, ya = R.avgpool_fwd(xc.double(), r)
    check('AvgPoolFn', nhwc(y), yr, ya, r * r, dtype)
    assert sink.passthrough(cl(pre).contiguous(memory_format=torch.channels_last)) is None   # first of two contributions
    y.backward(cl(dyc))
    dxr, dxa = R.avgpool_bwd(dyc.double(), H, W, r)
    check('AvgPoolFn_bwd', nhwc(x.grad), dxr + pre.double(), dxa + pre.double().abs(), 4, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_resize_fn_into_slice(dtype):
    from dmayolo.functional import ResizeFn, concat_buffer
    N, IH, IW, C, OH, OW = 2, 5, 7, 16, 10, 14
    gen = gen_for(2)
    xc, dyc = randn((N, IH, IW, C), gen, dtype), randn((N, OH, OW, C), gen, dtype)
    x = cl(xc).requires_grad_(True)
    buf = concat_buffer(N, 2 * C, OH, OW, x.detach()).fill_(FILL)
    y = ResizeFn.apply(x, OH, OW, [buf[:, C:]])
    assert y.data_ptr() == buf[:, C:].data_ptr() and bool((buf[:, :C] == FILL).all())
    assert equal(nhwc(y), R.resize_fwd(xc.double(), OH, OW)[0])
    gb, gs = slab(dyc, 24, 8)
    y.backward(gs.permute(0, 3, 1, 2))               # a strided upstream gradient
    dxr, dxa = R.resize_bwd(dyc.double(), IH, IW)
    check('ResizeFn_bwd', nhwc(x.grad), dxr, dxa, 4, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_scgate_fn(dtype):
    from dmayolo.functional import SCGateFn, GradSink
    N, H, W, C, GH, GW = 2, 17, 23, 16, 4, 5
    gen = gen_for(3)
    xc, gc = grid((N, H, W, C), gen, -64, 64, 1 / 16, dtype), grid((N, GH, GW, C), gen, -64, 64, 1 / 16, dtype)
    uc, dc, pre = randn((N, H, W, C), gen, dtype), randn((N, H, W, C), gen, dtype), randn((N, H, W, C), gen, dtype)
    x, u3, g = (cl(t).requires_grad_(True) for t in (xc, uc, gc))
    sink = GradSink(2)
    out = SCGateFn.apply(x, u3, g, sink)
    assert sink.passthrough(cl(pre).contiguous(memory_format=torch.channels_last)) is None
    out.backward(cl(dc))
    du3r, dprer, a3, ap = R.scgate_bwd(xc.double(), uc.double(), gc.double(), dc.double(), dtype)
    check('SCGateFn_du3', nhwc(u3.grad), du3r, a3, 4, dtype, trans=True)
    # the gate stores dpre in the storage type, then the sink adds it to the earlier contribution and the resize
    # backward sums it per pooled pixel: one more storage rounding of dpre on top of the final one (bf16), and in the
    # sum of n sigmoid-bearing terms each term brings its own 1e-5 (1 + |term|)
    st = R.BF16_STORE if dtype == BF16 else 0.0
    check('SCGateFn_dx', nhwc(x.grad), dprer + pre.double(), ap + pre.double().abs(), 4, dtype, trans=True, extra=st * ap)
    dgr, dga = R.resize_bwd(dprer, GH, GW)
    n = R.resize_max_preimage(GH, GW, H, W)
    check('SCGateFn_dg', nhwc(g.grad), dgr, dga, n, dtype, extra=st * dga + R.TRANS * (n + dga))


@pytest.mark.parametrize('dtype', DTYPES)
def test_coorattention_fns(dtype):
    from dmayolo.functional import CAPoolFn, CAApplyFn
    N, H, W, C = 2, 5, 9, 6
    gen = gen_for(4)
    xc = randn((N, H, W, C), gen, dtype)
    xbuf, xs = slab(xc, 16, 8)
    x = xs.permute(0, 3, 1, 2).requires_grad_(True)
    y = CAPoolFn.apply(x)                                          # [N, C, H + W, 1]
    yr, ya = R.ca_pool_fwd(xc.double())
    assert tuple(y.shape) == (N, C, H + W, 1)
    check('CAPoolFn', y[..., 0].permute(0, 2, 1), yr, ya, max(H, W), dtype)
    dyc = randn((N, H + W, C), gen, dtype)
    y.backward(dyc.cuda().permute(0, 2, 1)[..., None])
    dxr, dxa = R.ca_pool_bwd(dyc.double(), H, W)
    check('CAPoolFn_bwd', nhwc(x.grad), dxr, dxa, 4, dtype)

    x.grad = None
    lhc = (torch.rand((N, H + W, C), generator=gen) * 16 - 8).to(dtype)
    lwc = (torch.rand((N, H + W, C), generator=gen) * 16 - 8).to(dtype)
    lh = lhc.cuda().permute(0, 2, 1)[..., None].requires_grad_(True)
    lw = lwc.cuda().permute(0, 2, 1)[..., None].requires_grad_(True)
    out = CAApplyFn.apply(x, lh, lw)
    outr, outa = R.ca_apply_fwd(xc.double(), lhc.double(), lwc.double())
    check('CAApplyFn', nhwc(out), outr, outa, 4, dtype, trans=True)
    doc = randn((N, H, W, C), gen, dtype)
    gb, gs = slab(doc, 16, 8)
    out.backward(gs.permute(0, 3, 1, 2))
    dxr, dlhr, dlwr, dxa, alh, alw = R.ca_apply_bwd(xc.double(), lhc.double(), lwc.double(), doc.double())
    check('CAApplyFn_dx', nhwc(x.grad), dxr, dxa, 4, dtype, trans=True)
    check('CAApplyFn_dlh', lh.grad[..., 0].permute(0, 2, 1), dlhr, alh, max(H, W) + 5, dtype, trans=True)
    check('CAApplyFn_dlw', lw.grad[..., 0].permute(0, 2, 1), dlwr, alw, max(H, W) + 5, dtype, trans=True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_cbam_fns(dtype):
    from dmayolo.functional import HalvesSigmoidFn, CBAMInFn, PixScaleFn, GradSink
    N, H, W, C = 2, 5, 14, 16
    HW = H * W
    gen = gen_for(5)
    zc, dcc = grid((2 * N, C), gen, -64, 64, 1 / 16, dtype), randn((N, C), gen, dtype)
    z = zc.cuda()[..., None, None].requires_grad_(True)
    ca = HalvesSigmoidFn.apply(z)
    car = R.halves_sigmoid_fwd(zc.double(), dtype)
    check('HalvesSigmoidFn', ca.flatten(1), car, car, 4, dtype, trans=True)
    ca.backward(dcc.cuda()[..., None, None])
    dzr = R.halves_sigmoid_bwd(zc.double(), dcc.double(), dtype)
    check('HalvesSigmoidFn_bwd', z.grad.flatten(1), dzr, dzr.abs(), 4, dtype, trans=True)

    xc, cac = grid((N, H, W, C), gen, -8, 8, 1 / 4, dtype), grid((N, C), gen, 1, 8, 1 / 8, dtype)
    xbuf, xs = slab(xc, 24, 8)
    x = xs.permute(0, 3, 1, 2).requires_grad_(True)
    cav = cac.cuda()[..., None, None].requires_grad_(True)
    sink = GradSink(2)
    out1, s2 = CBAMInFn.apply(x, cav, sink)
    o1r, meanr, mxr, amr, ma = R.cbam_in_fwd(xc.double().view(N, HW, C), cac.double(), dtype)
    assert equal(nhwc(out1), o1r.view(N, H, W, C)) and equal(s2[:, 1], mxr.view(N, H, W))
    check('CBAMInFn_mean', s2[:, 0], meanr.view(N, H, W), ma.view(N, H, W), C, dtype)
    d1c, ds2c, pre = randn((N, H, W, C), gen, dtype), randn((N, H, W, 2), gen, dtype), randn((N, H, W, C), gen, dtype)
    assert sink.passthrough(cl(pre).contiguous(memory_format=torch.channels_last)) is None
    torch.autograd.backward([out1, s2], [cl(d1c), cl(ds2c)])
    dxr, dcar, dxa, dcaa = R.cbam_in_bwd(xc.double().view(N, HW, C), cac.double(), d1c.double().view(N, HW, C),
                                         ds2c.double().view(N, HW, 2), amr)
    base = pre.double().view(N, HW, C)
    check('CBAMInFn_dx', nhwc(x.grad).reshape(N, HW, C), dxr + base, dxa + base.abs(), 4, dtype)
    check('CBAMInFn_dca', cav.grad.flatten(1), dcar, dcaa, HW + 4, dtype)

    sac = torch.rand((N, H, W, 1), generator=gen).to(dtype)
    o1 = cl(o1r.view(N, H, W, C).to(dtype)).requires_grad_(True)
    sa = cl(sac).requires_grad_(True)
    out = PixScaleFn.apply(o1, sa)
    outr, outa = R.pixscale_fwd(o1r, sac.double().view(N, HW))
    check('PixScaleFn', nhwc(out).reshape(N, HW, C), outr, outa, 4, dtype)
    out.backward(cl(d1c))
    g1r, dsar, g1a, dsaa = R.pixscale_bwd(o1r, sac.double().view(N, HW), d1c.double().view(N, HW, C))
    check('PixScaleFn_dout1', nhwc(o1.grad).reshape(N, HW, C), g1r, g1a, 4, dtype)
    check('PixScaleFn_dsa', sa.grad.reshape(N, HW), dsar, dsaa, C + 1, dtype)


# ---------------------------------------------------------------- slice copy and the image source kinds
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,Ct,off', LAYOUTS)
@pytest.mark.parametrize('acc', [0, 1])
def test_slice_copy(acc, C, Ct, off, dtype):
    """dst (+)= src * w[idx] / (sum w + eps) between channel slices of wider buffers, in the vector and the scalar form
    (LAYOUTS).  The scale is three fp32 additions and a division, then one product and one sum per element: n = 8."""
    call, ptr, stream = _lib()
    M, eps = 37, 1e-4
    gen = gen_for(C, Ct, off, acc)
    sc_, g0 = randn((M, C), gen, dtype), randn((M, C), gen, dtype)
    w = torch.rand(3, generator=gen) + 0.5
    sbuf, src = slab(sc_, Ct, off)
    dbuf, dst = slab(g0, Ct, off)
    wd = w.cuda()
    call('dmy_slice_copy', dcode(dtype), ptr(src), Ct, ptr(dst), Ct, M, C, ptr(wd), 1, 3, eps, acc, stream())
    t = sc_.double() * (w[1].double() / (w.double().sum() + eps))
    base = g0.double() * acc
    check(f'slice_copy_acc{acc}', dst, t + base, t.abs() + base.abs(), 8, dtype)
    assert untouched(dbuf, off, C) and untouched(sbuf, off, C)


@pytest.mark.parametrize('dtype', DTYPES)
def test_image_s2d_source_kinds(dtype):
    """dmy_image_s2d reads a uint8 or an fp32 NCHW image: both convert to fp32 exactly before the one product with
    `scale`, so the two give the same bits; the layout is that of the reference's space-to-depth cat, zero padded"""
    call, ptr, stream = _lib()
    N, C, H, W, Cs, scale = 2, 3, 6, 10, 16, 1 / 255
    x8 = torch.randint(0, 256, (N, C, H, W), generator=gen_for(C, H), dtype=torch.uint8).cuda()
    outs = []
    for kind, x in ((0, x8), (1, x8.float())):
        y = torch.full((N, H // 2, W // 2, Cs), FILL, dtype=dtype, device='cuda')
        call('dmy_image_s2d', dcode(dtype), kind, ptr(x), ptr(y), N, C, H, W, Cs, scale, stream())
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    xf = (x8.float() * torch.tensor(scale, dtype=torch.float32)).to(dtype)
    cat = torch.cat([xf[..., dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], 1).permute(0, 2, 3, 1)
    assert torch.equal(outs[0][..., :4 * C], cat) and bool((outs[0][..., 4 * C:] == 0).all())
