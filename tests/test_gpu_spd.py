"""GPU: the kernels of csrc/spd.hip, bf16 and fp32.  They move data and reuse the math of existing passes, so the checks
are exact equalities: each fused pass against the launches it replaces, the 2 x 2 max pool against torch's CPU
max_pool2d and its autograd.  Only the folded sums of the backward reduce are also held to a float64 reference.

Shapes (N, H, W, C): one vector with W / 2 odd, three vectors, one output pixel, and (2, 34, 38, 32), where the
row-mapped passes run several blocks (6 or 11 partial rows in the reduce); each once dense and once with the SM-side tensor a
slice at channel offset 8 of a wider buffer whose other channels must stay untouched.

Reduce bound.  No test here checks dmy_bn_bwd_reduce against float64 on its own, so the bound is derived: a term
t = dy * act'(u) [* xhat] is a handful of fp32 roundings plus the v_exp_f32 / v_rcp_f32 sigmoid, whose exponent argument
carries up to |u| * 2^-24 of absolute error, at most 2^-18 relative for |u| < 64.  A sum passes through at most 8
additions per thread (a block covers eight row groups' worth of rows), 256 across the block's row groups and 11 across
the partial rows here, under 2^9 additions of 2^-24 each relative to sum |t|.  Bound per channel: (2^-15 + 2^-18) *
sum_m |t_m|, with t computed in float64 from the same inputs.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32, BF16 = torch.float32, torch.bfloat16
ACT_NONE, ACT_SILU, ACT_LEAKY = 0, 1, 6
SENTINEL = 7.0


def _shapes(dtype):
    return [(2, 6, 10, 8 if dtype == BF16 else 4), (2, 6, 10, 24), (1, 2, 2, 16), (2, 34, 38, 32)]


CASES = [(dt, i, wide) for dt in (F32, BF16) for i in range(4) for wide in (False, True)]
IDS = [f'{str(dt)[6:]}-s{i}-{"slice" if wide else "dense"}' for dt, i, wide in CASES]


def _nhwc(n, c, h, w, dtype, gen, ints=False):
    t = torch.randint(-3, 4, (n, c, h, w), generator=gen).float() if ints else torch.randn(n, c, h, w, generator=gen)
    return t.to(dtype).cuda().contiguous(memory_format=CL)


def _sm_buf(n, c4, h2, w2, dtype, wide, src=None):
    """-> (the SM-side tensor, its buffer or None): dense, or channels 8 .. 8 + c4 of a buffer 16 channels wider that is
    filled with a sentinel"""
    if not wide:
        t = torch.empty(n, c4, h2, w2, dtype=dtype, device='cuda').contiguous(memory_format=CL)
        if src is not None:
            t.copy_(src)
        return t, None
    buf = torch.full((n, c4 + 16, h2, w2), SENTINEL, dtype=dtype, device='cuda').contiguous(memory_format=CL)
    t = buf[:, 8:8 + c4]
    if src is not None:
        t.copy_(src)
    return t, buf


def _untouched(buf, c4):
    if buf is not None:
        assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + c4:] == SENTINEL).all())


def _coef(K, gen):
    return [(torch.rand(K, generator=gen) + 0.5).cuda(), (torch.randn(K, generator=gen) * 0.3).cuda(),
            (torch.randn(K, generator=gen) * 0.2).cuda(), (torch.rand(K, generator=gen) + 0.5).cuda()]


def _fn():
    import dmayolo.functional as Fn
    return Fn, Fn.call, Fn.ptr, Fn.stream


@pytest.mark.parametrize('dtype,si,wide', CASES, ids=IDS)
def test_bn_act_s2d_fwd_equals_bn_act_then_space_to_depth(dtype, si, wide):
    Fn, call, ptr, stream = _fn()
    N, H, W, K = _shapes(dtype)[si]
    gen = torch.Generator().manual_seed(si)
    z = _nhwc(N, K, H, W, dtype, gen)
    scale, shift, _, _ = _coef(K, gen)
    dt = Fn.DT[dtype]
    for act in (ACT_SILU, ACT_LEAKY, ACT_NONE):
        y, buf = _sm_buf(N, 4 * K, H // 2, W // 2, dtype, wide)
        call('dmy_bn_act_s2d_fwd', dt, ptr(z), K, ptr(scale), ptr(shift), act, ptr(y), Fn.pixel_stride(y)[1], N, H, W, K, stream())
        t = torch.empty_like(z)
        call('dmy_bn_act_fwd', dt, ptr(z), K, ptr(scale), ptr(shift), act, None, 0, ptr(t), K, N * H * W, K, stream())
        ref = torch.empty(N, 4 * K, H // 2, W // 2, dtype=dtype, device='cuda').contiguous(memory_format=CL)
        call('dmy_space_to_depth', dt, ptr(t), K, ptr(ref), 4 * K, N, H, W, K, 0, stream())
        torch.cuda.synchronize()
        assert torch.equal(y, ref), act
        _untouched(buf, 4 * K)
        # and the layout is the reference's cat
        cat = torch.cat([t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]], 1)
        assert torch.equal(y, cat)


@pytest.mark.parametrize('dtype,si,wide', CASES, ids=IDS)
def test_bn_bwd_s2d_passes(dtype, si, wide):
    """apply: bit for bit dmy_space_to_depth(backward) then dmy_bn_bwd_apply.  reduce: the partial rows are those of
    dmy_bn_bwd_reduce over the un-SM'd gradient bit for bit, two runs are bit-identical, and the folded sums are within
    the module docstring's bound of float64 column sums"""
    Fn, call, ptr, stream = _fn()
    N, H, W, K = _shapes(dtype)[si]
    M = N * H * W
    gen = torch.Generator().manual_seed(10 + si)
    z = _nhwc(N, K, H, W, dtype, gen)
    dsrc = _nhwc(N, 4 * K, H // 2, W // 2, dtype, gen)
    dy, buf = _sm_buf(N, 4 * K, H // 2, W // 2, dtype, wide, dsrc)
    dps = Fn.pixel_stride(dy)[1]
    stats = _coef(K, gen)  # scale, shift, mean, invstd
    coef = [(torch.randn(K, generator=gen) * 0.5).cuda() for _ in range(3)]
    dt = Fn.DT[dtype]
    full = torch.empty_like(z)  # SM^-1(dy)
    call('dmy_space_to_depth', dt, ptr(full), K, ptr(dy), dps, N, H, W, K, 1, stream())
    for act in (ACT_SILU, ACT_NONE):
        dz, ref = torch.empty_like(z), torch.empty_like(z)
        call('dmy_bn_bwd_apply_s2d', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), act, *map(ptr, coef), ptr(dz), K,
             N, H, W, K, stream())
        call('dmy_bn_bwd_apply', dt, ptr(z), K, ptr(full), K, *map(ptr, stats), act, *map(ptr, coef), ptr(ref), K, M, K,
             stream())
        torch.cuda.synchronize()
        assert torch.equal(dz, ref), act
        P = call('dmy_bn_bwd_reduce_s2d_rows', dt, M, K)
        assert P == call('dmy_bn_reduce_rows', dt, ptr(z), K, ptr(full), K, M, K) and (P > 1) == (si == 3)
        runs = []
        for _ in range(2):
            pdb, pdg = torch.full((P, K), float('nan'), device='cuda'), torch.full((P, K), float('nan'), device='cuda')
            call('dmy_bn_bwd_reduce_s2d', dt, ptr(z), K, ptr(dy), dps, *map(ptr, stats), act, N, H, W, K, ptr(pdb),
                 ptr(pdg), stream())
            runs.append((pdb, pdg))
        rdb, rdg = torch.empty(P, K, device='cuda'), torch.empty(P, K, device='cuda')
        call('dmy_bn_bwd_reduce', dt, ptr(z), K, ptr(full), K, *map(ptr, stats), act, M, K, ptr(rdb), ptr(rdg), stream())
        torch.cuda.synchronize()
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(runs[0][0], rdb) and torch.equal(runs[0][1], rdg)
        fa, fb, rows = Fn._fold_partials(runs[0][0].view(-1), runs[0][1].view(-1), P, K, z.device)
        got_b, got_g = fa.view(rows, K).double().sum(0).cpu(), fb.view(rows, K).double().sum(0).cpu()
        sc, sh, mu, inv = (t.double().cpu().view(1, K, 1, 1) for t in stats)
        zd, gd = z.double().cpu(), full.double().cpu()
        u = zd * sc + sh
        s = torch.sigmoid(u)
        du = gd * (s * (1 + u * (1 - s)) if act == ACT_SILU else torch.ones_like(u))
        tb, tg = du, du * (zd - mu) * inv
        for got, t in ((got_b, tb), (got_g, tg)):
            ref_sum, bound = t.sum((0, 2, 3)), (2.0 ** -15 + 2.0 ** -18) * t.abs().sum((0, 2, 3))
            print('reduce act %d max err / bound %.3g' % (act, float(((got - ref_sum).abs() / bound).max())))
            assert bool(((got - ref_sum).abs() <= bound).all())
    _untouched(buf, 4 * K)
    assert torch.equal(dy, dsrc)


POOL_SHAPES = [(2, 6, 10, 8), (2, 6, 10, 24), (1, 2, 2, 16), (2, 5, 7, 8)]


def _pool_input(n, h, w, c, dtype, gen):
    """integer values in -3 .. 3 (ties in most windows), one window holding a NaN next to a larger value"""
    x = torch.randint(-3, 4, (n, c, h, w), generator=gen).float()
    x[0, 0, 0, 0], x[0, 0, 1, 1] = 3.0, float('nan')
    x[0, 1, 0, :2], x[0, 1, 1, :2] = 2.0, 2.0  # a four-way tie: the first tap wins
    return x


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool2_equals_torch_cpu(dtype, shape):
    Fn, call, ptr, stream = _fn()
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(H * W + C)
    xc = _pool_input(N, H, W, C, dtype, gen).requires_grad_(True)
    yr = F.max_pool2d(xc, 2, 2)
    gup = torch.randint(-3, 4, yr.shape, generator=gen).float()
    (dxr,) = torch.autograd.grad(yr, xc, gup)
    x = xc.detach().to(dtype).cuda().contiguous(memory_format=CL)
    OH, OW = H // 2, W // 2
    y = torch.empty(N, C, OH, OW, dtype=dtype, device='cuda').contiguous(memory_format=CL)
    arg = torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device='cuda')
    dt = Fn.DT[dtype]
    call('dmy_maxpool2_fwd', dt, ptr(x), C, ptr(y), C, ptr(arg), N, H, W, C, stream())
    torch.testing.assert_close(y.float().cpu(), yr.detach(), rtol=0, atol=0, equal_nan=True)
    assert int(arg.max()) <= 3 and int(arg[0, 0, 0, 0]) == 3 and int(arg[0, 0, 0, 1]) == 0
    assert bool(torch.isnan(y[0, 0, 0, 0]))
    dy = gup.to(dtype).cuda().contiguous(memory_format=CL)
    pre = torch.randint(-3, 4, (N, C, H, W), generator=gen).float()
    for acc in (0, 1):
        dx = pre.to(dtype).cuda().contiguous(memory_format=CL)
        call('dmy_maxpool2_bwd', dt, ptr(dy), C, ptr(arg), ptr(dx), C, acc, N, H, W, C, stream())
        torch.testing.assert_close(dx.float().cpu(), dxr + acc * pre, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize('dtype,si,wide', CASES, ids=IDS)
def test_spd_split_equals_separate_kernels(dtype, si, wide):
    """forward: SM(x), MP(x) and the argmax of the two separate kernels bit for bit.  backward: the fp32 sum of the two
    gradients rounded once to storage"""
    Fn, call, ptr, stream = _fn()
    N, H, W, C = _shapes(dtype)[si]
    OH, OW = H // 2, W // 2
    gen = torch.Generator().manual_seed(20 + si)
    x = _pool_input(N, H, W, C, dtype, gen).to(dtype).cuda().contiguous(memory_format=CL)
    dt = Fn.DT[dtype]
    sm, buf = _sm_buf(N, 4 * C, OH, OW, dtype, wide)
    new = lambda c: torch.empty(N, c, OH, OW, dtype=dtype, device='cuda').contiguous(memory_format=CL)  # noqa: E731
    mp, mpr, smr = new(C), new(C), new(4 * C)
    arg, argr = (torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device='cuda') for _ in range(2))
    call('dmy_spd_split_fwd', dt, ptr(x), C, ptr(sm), Fn.pixel_stride(sm)[1], ptr(mp), C, ptr(arg), N, H, W, C, stream())
    call('dmy_space_to_depth', dt, ptr(x), C, ptr(smr), 4 * C, N, H, W, C, 0, stream())
    call('dmy_maxpool2_fwd', dt, ptr(x), C, ptr(mpr), C, ptr(argr), N, H, W, C, stream())
    torch.cuda.synchronize()
    as_int = lambda t: t.contiguous().view(torch.int16 if dtype == BF16 else torch.int32)  # noqa: E731  (NaN bits too)
    assert torch.equal(as_int(sm), as_int(smr)) and torch.equal(as_int(mp), as_int(mpr)) and torch.equal(arg, argr)
    _untouched(buf, 4 * C)
    dsrc = _nhwc(N, 4 * C, OH, OW, dtype, gen)
    dsm, dbuf = _sm_buf(N, 4 * C, OH, OW, dtype, wide, dsrc)
    dmp = _nhwc(N, C, OH, OW, dtype, gen)
    dx = torch.empty_like(x)
    call('dmy_spd_split_bwd', dt, ptr(dsm), Fn.pixel_stride(dsm)[1], ptr(dmp), C, ptr(arg), ptr(dx), C, N, H, W, C, stream())
    a, b = torch.empty_like(x), torch.empty_like(x)
    call('dmy_space_to_depth', dt, ptr(a), C, ptr(dsm), Fn.pixel_stride(dsm)[1], N, H, W, C, 1, stream())
    call('dmy_maxpool2_bwd', dt, ptr(dmp), C, ptr(arg), ptr(b), C, 0, N, H, W, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(dx, (a.float() + b.float()).to(dtype))
    _untouched(dbuf, 4 * C)


def test_unsupported_arguments_launch_nothing():
    Fn, call, ptr, stream = _fn()
    x = torch.zeros(1, 8, 4, 4, device='cuda', dtype=BF16).contiguous(memory_format=CL)
    y = torch.zeros(1, 32, 2, 2, device='cuda', dtype=BF16).contiguous(memory_format=CL)
    one = torch.ones(8, device='cuda')
    with pytest.raises(RuntimeError, match='dmy_bn_act_s2d_fwd failed'):  # odd height
        call('dmy_bn_act_s2d_fwd', 1, ptr(x), 8, ptr(one), ptr(one), 0, ptr(y), 32, 1, 3, 4, 8, stream())
    with pytest.raises(RuntimeError, match='dmy_spd_split_fwd failed'):  # 12 channels are not whole bf16 vectors
        call('dmy_spd_split_fwd', 1, ptr(x), 12, ptr(y), 48, ptr(y), 12, ptr(y), 1, 4, 4, 12, stream())
    with pytest.raises(NotImplementedError, match='multiples of 8'):
        Fn.MaxPool2Fn.apply(torch.zeros(1, 12, 4, 4, device='cuda', dtype=BF16).contiguous(memory_format=CL))
    assert float(y.abs().sum()) == 0.0
