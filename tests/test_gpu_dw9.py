"""GPU: the depthwise 9x9 stride-1 conv with bias (csrc/dwconv.hip, the first layer of ConvMix.Resnet, models/cspcm.py:29)
through the C ABI against float64 torch on the same storage-rounded operands, bf16 and fp32.  Cases: the three shapes of
tests/golden/dw9.npz -- (2, 8, 5, 7), the whole map inside the halo; (1, 24, 9, 13), three channel units and W no
multiple of the strip; (2, 16, 12, 18) -- whose recorded fp32 results must agree with the float64 computation to 1e-5
rel-L2, and a seeded (2, 16, 11, 14) case read from and written to channels [32, 48) of 64-channel buffers.

Bounds: those derived in tests/test_gpu_dw7.py's docstring, carried over with 81 taps.
fp32 forward / data-grad / weight-grad: rel-L2 against float64 at most 4x that of torch's own fp32 conv on the same input.
bf16 forward / data-grad, per element: 81 exact products, at most 82 fp32 additions (bias included), 82 * 2^-24 < 2^-18
relative to sum |x w| + |b|, then one rounding to bf16: 2^-8 |ref| + 2^-18 (sum |x w| + |b|).
Weight-grad taps (both dtypes): under 2^6 roundings of 2^-24 relative to sum |t|: 2^-18 * sum |t|.
Every output lies in a guard band that must stay untouched, and a second run must be bit-identical."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_dw7 import _guarded, _guard_ok, _nhwc, _rest_ok, _rel, _wop, _check_map

pytestmark = pytest.mark.gpu

CL = torch.channels_last
K, P = 9, 4
# (N, C, H, W, Ct, c0): the last one is a slice of a wider buffer (pixel stride 64 > C)
SHAPES = [(2, 8, 5, 7, 8, 0), (1, 24, 9, 13, 24, 0), (2, 16, 12, 18, 16, 0), (2, 16, 11, 14, 64, 32)]
CASES = [(dt, i) for dt in (torch.float32, torch.bfloat16) for i in range(4)]
IDS = [f'{str(dt)[6:]}-s{i}' for dt, i in CASES]
_CACHE, _GOLD = {}, []


def _gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dw9.npz')))
    return _GOLD[0]


def _case(dtype, i):
    key = (dtype, i)
    if key not in _CACHE:
        N, C, H, W, Ct, c0 = SHAPES[i]
        gold = None
        if i < 3:
            gold = {k: torch.from_numpy(_gold()[f'{i}.{k}']) for k in ('x', 'w', 'b', 'dz', 'y', 'dx', 'dw', 'db')}
            x, w, b, dz = gold['x'], gold['w'], gold['b'], gold['dz']
            assert tuple(x.shape) == (N, C, H, W)
        else:
            g = torch.Generator().manual_seed(900 + i)
            x, w = torch.randn(N, C, H, W, generator=g), torch.randn(C, 1, K, K, generator=g) / K
            b, dz = torch.randn(C, generator=g), torch.randn(N, C, H, W, generator=g)
        x, w, b, dz = x.to(dtype).cuda(), w.cuda(), b.cuda(), dz.to(dtype).cuda()
        xd, wd, zd = x.double(), w.to(dtype).double(), dz.double()
        ref = dict(
            y=F.conv2d(xd, wd, b.double(), padding=P, groups=C),
            ymag=F.conv2d(xd.abs(), wd.abs(), b.double().abs(), padding=P, groups=C),
            dx=torch.nn.grad.conv2d_input((N, C, H, W), wd, zd, padding=P, groups=C),
            dxmag=torch.nn.grad.conv2d_input((N, C, H, W), wd.abs(), zd.abs(), padding=P, groups=C),
            dw=torch.nn.grad.conv2d_weight(xd, (C, 1, K, K), zd, padding=P, groups=C),
            dwmag=torch.nn.grad.conv2d_weight(xd.abs(), (C, 1, K, K), zd.abs(), padding=P, groups=C))
        t32 = None
        if dtype == torch.float32:
            if gold is not None:
                for k in ('y', 'dx', 'dw'):
                    assert _rel(gold[k].cuda(), ref[k]) < 1e-5, k
            t32 = dict(y=F.conv2d(x, w, b, padding=P, groups=C),
                       dx=torch.nn.grad.conv2d_input((N, C, H, W), w, dz, padding=P, groups=C),
                       dw=torch.nn.grad.conv2d_weight(x, (C, 1, K, K), dz, padding=P, groups=C))
        _CACHE[key] = (x, w, b, dz, ref, t32)
    return _CACHE[key]


def _geo(i):
    N, C, H, W, Ct, c0 = SHAPES[i]
    return (N, H, W, C, Ct, K, K, 1, P, H, W, Ct)


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw9_fwd(dtype, i):
    """dmy_dwconv_fwd: z = T(conv + bias) with its partial rows (sums of the values as stored), and without them"""
    from dmayolo.functional import call, ptr, stream
    N, C, H, W, Ct, c0 = SHAPES[i]
    x, w, b, _, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    xf, xb, xv = _nhwc(x, Ct, c0)
    wd = _wop(w, dtype)
    assert call('dmy_dwconv_ok', dt, ptr(xv), ptr(wd), ptr(xv), N, H, W, C, C, C, Ct, K, K, 1, P, H, W, Ct) == 1
    rows = call('dmy_dwconv_fwd_rows', N * H * W, C)
    outs = []
    for run in range(2):
        zf, zb, zv = _nhwc(torch.full_like(x, float('nan')), Ct, c0)
        pf, ps = _guarded((rows, C), torch.float32)
        qf, pq = _guarded((rows, C), torch.float32)
        ps.fill_(float('nan')), pq.fill_(float('nan'))
        call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(b), ptr(zv), ptr(ps), ptr(pq), *_geo(i), stream())
        torch.cuda.synchronize()
        assert _rest_ok(zf, zb, C, c0) and _rest_ok(xf, xb, C, c0) and _guard_ok(pf) and _guard_ok(qf)
        assert torch.isfinite(zv).all() and torch.isfinite(ps).all() and torch.isfinite(pq).all()
        outs.append((zv.clone(), ps.clone(), pq.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*outs))
    z, ps, pq = outs[0]
    _check_map('fwd', z, ref['y'], ref['ymag'], t32 and t32['y'], dtype)
    stored = z.double()
    assert _rel(pq.sum(0), (stored ** 2).sum((0, 2, 3))) < 1e-5
    assert float((ps.sum(0).double() - stored.sum((0, 2, 3))).abs().max()) <= 2.0 ** -18 * float(stored.abs().sum((0, 2, 3)).max())
    z2 = torch.full_like(x, float('nan')).contiguous(memory_format=CL)
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(b), ptr(z2), None, None, N, H, W, C, Ct, K, K, 1, P, H, W, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(z2, z)


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw9_dgrad_and_accumulate(dtype, i):
    from dmayolo.functional import call, ptr, stream
    N, C, H, W, Ct, c0 = SHAPES[i]
    x, w, _, dz, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    zf, zb, zv = _nhwc(dz, Ct, c0)
    wd = _wop(w, dtype)
    outs = []
    for run in range(2):
        df, db_, dv = _nhwc(torch.full_like(dz, float('nan')), Ct, c0)
        call('dmy_dwconv_dgrad', dt, ptr(zv), ptr(wd), ptr(dv), 0, *_geo(i), stream())
        torch.cuda.synchronize()
        assert _rest_ok(df, db_, C, c0) and _rest_ok(zf, zb, C, c0) and torch.isfinite(dv).all()
        outs.append(dv.clone())
    assert torch.equal(outs[0], outs[1])
    _check_map('dgrad', outs[0], ref['dx'], ref['dxmag'], t32 and t32['dx'], dtype)
    if i == 3:  # accumulate = 1: dx = T(dx0 + acc), one more rounding of the sum
        af, ab, av = _nhwc(x, Ct, c0)
        call('dmy_dwconv_dgrad', dt, ptr(zv), ptr(wd), ptr(av), 1, *_geo(i), stream())
        torch.cuda.synchronize()
        assert _rest_ok(af, ab, C, c0)
        want = x.double() + ref['dx']
        if dtype == torch.float32:
            assert _rel(av, want) <= 4 * _rel(x + t32['dx'], want)
        else:
            bound = 2.0 ** -8 * want.abs() + 2.0 ** -18 * (x.double().abs() + ref['dxmag'])
            assert float(((av.double() - want).abs() / bound).max()) <= 1.0


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw9_wgrad(dtype, i):
    from dmayolo.functional import call, ptr, stream
    N, C, H, W, Ct, c0 = SHAPES[i]
    x, _, _, dz, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    _, _, xv = _nhwc(x, Ct, c0)
    _, _, zv = _nhwc(dz, Ct, c0)
    rows = call('dmy_dwconv_wgrad_rows', N * H * W, C)
    outs = []
    for run in range(2):
        pf, part = _guarded((rows, K * K * C), torch.float32)
        part.fill_(float('nan'))
        wf, dw = _guarded((C, 1, K, K), torch.float32)
        call('dmy_dwconv_wgrad', dt, ptr(xv), ptr(zv), ptr(part), *_geo(i), stream())
        call('dmy_dwconv_wgrad_finalize', ptr(part), rows, C, K, K, ptr(dw), 0, stream())
        torch.cuda.synchronize()
        assert _guard_ok(pf) and _guard_ok(wf)
        assert torch.isfinite(part).all(), 'every partial row must be written'
        outs.append(dw.clone())
    assert torch.equal(outs[0], outs[1])
    ew = float(((outs[0].double() - ref['dw']).abs() / (2.0 ** -18 * ref['dwmag']).clamp_min(1e-300)).max())
    print(f'{dtype} wgrad max err / bound {ew:.3g}, rows {rows}')
    assert ew <= 1.0, ew
    if dtype == torch.float32:
        own, err = _rel(t32['dw'], ref['dw']), _rel(outs[0], ref['dw'])
        print(f'fp32 wgrad: torch {own:.2e} kernel {err:.2e}')
        assert err <= 4 * own, (err, own)
    with pytest.raises(RuntimeError):  # the bias weight-grad stays k = 7 only
        call('dmy_dwconv_wgrad_bias', dt, ptr(xv), ptr(zv), ptr(part), *_geo(i), stream())


@pytest.mark.parametrize('dtype,i', [(torch.float32, 1), (torch.bfloat16, 1), (torch.float32, 3), (torch.bfloat16, 3)],
                         ids=['float32-s1', 'bfloat16-s1', 'float32-s3', 'bfloat16-s3'])
def test_dw9_fwd_actbn(dtype, i):
    """dmy_dwconv_fwd_actbn against GELU(dmy_dwconv_fwd's z) * scale + shift + res in float64.  The epilogue's fp32
    arithmetic and one storage rounding give ulp(T) / 2 * |y| + 2^-20 (|a * scale| + |shift| + |res|).  The two launches
    are different instantiations, so their pre-activations need not agree bit for bit: each lies within the forward
    bound 2^-18 (sum |x w| + |b|) of the exact sum (a z that is small by cancellation differs by far more than its own
    ulp; measured 4e-5 relative at z = -1.4e-3 in fp32), and in bf16 the two roundings of z may fall on either side of a
    tie, one ulp = 2^-7 |z|.  GELU' <= 1.13, so the term 1.13 |scale| (2^-17 (sum |x w| + |b|) + [bf16] 2^-7 |z|) is
    added."""
    from dmayolo.functional import call, ptr, stream, ACT_GELU
    N, C, H, W, Ct, c0 = SHAPES[i]
    x, w, b, dz, ref, _ = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    g = torch.Generator().manual_seed(19)
    scale, shift = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    wd = _wop(w, dtype)
    _, _, xv = _nhwc(x, Ct, c0)
    _, _, rv = _nhwc(dz, Ct, c0)  # residual
    _, _, zv = _nhwc(torch.zeros_like(x), Ct, c0)
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(b), ptr(zv), None, None, *_geo(i), stream())
    outs = []
    for run in range(2):
        yf, yb, yv = _nhwc(torch.full_like(x, float('nan')), Ct, c0)
        call('dmy_dwconv_fwd_actbn', dt, ptr(xv), ptr(wd), ptr(b), ptr(yv), *_geo(i), ptr(scale), ptr(shift), ACT_GELU,
             ptr(rv), Ct, stream())
        torch.cuda.synchronize()
        assert _rest_ok(yf, yb, C, c0) and torch.isfinite(yv).all()
        outs.append(yv.clone())
    assert torch.equal(outs[0], outs[1])
    a = F.gelu(zv.double())
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    want = a * sc + sh + rv.double()
    half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    zerr = 1.13 * (2.0 ** -17 * ref['ymag'] + (2.0 ** -7 * zv.double().abs() if dt else 0.0))
    bound = half_ulp * want.abs() + 2.0 ** -20 * ((a * sc).abs() + sh.abs() + rv.double().abs()) + sc.abs() * zerr
    worst = float(((outs[0].double() - want).abs() / bound).max())
    print(f'{dtype} fwd_actbn max err / bound {worst:.3g}')
    assert worst <= 1.0, worst
    # without the affine map and the residual: GELU(z) alone
    y0 = torch.full_like(x, float('nan')).contiguous(memory_format=CL)
    call('dmy_dwconv_fwd_actbn', dt, ptr(xv), ptr(wd), ptr(b), ptr(y0), N, H, W, C, Ct, K, K, 1, P, H, W, C, None, None,
         ACT_GELU, None, 0, stream())
    torch.cuda.synchronize()
    ratio = (y0.double() - a).abs() / (half_ulp * a.abs() + 2.0 ** -20 * zv.double().abs() + zerr + 1e-30)
    j = int(ratio.flatten().argmax())
    print(f'{dtype} gelu-only max err / bound {float(ratio.max()):.3g} at z = {float(zv.flatten()[j]):.6g}: got '
          f'{float(y0.flatten()[j]):.9g} want {float(a.flatten()[j]):.9g}')
    assert float(ratio.max()) <= 1.0


def test_dw9_rejected_geometries_launch_nothing():
    """9x9 at stride 2, 12 bf16 channels, fwd_actbn at k = 7: the query says 0 / the entries return -1 (call() raises)
    and write nothing"""
    from dmayolo.functional import call, ptr, stream
    x = torch.zeros(1, 16, 12, 12, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)
    y = torch.full((1, 16, 12, 12), float('nan'), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)
    w = torch.zeros(81, 16, dtype=torch.bfloat16, device='cuda')
    part = torch.full((1, 81 * 16), float('nan'), device='cuda')
    assert call('dmy_dwconv_ok', 1, ptr(x), ptr(w), ptr(y), 1, 12, 12, 16, 16, 16, 16, 9, 9, 2, 4, 6, 6, 16) == 0
    assert call('dmy_dwconv_ok', 1, ptr(x), ptr(w), ptr(y), 1, 12, 12, 12, 12, 12, 16, 9, 9, 1, 4, 12, 12, 16) == 0
    for geo in ((1, 12, 12, 16, 16, 9, 9, 2, 4, 6, 6, 16), (1, 12, 12, 12, 16, 9, 9, 1, 4, 12, 12, 16)):
        with pytest.raises(RuntimeError):
            call('dmy_dwconv_fwd', 1, ptr(x), ptr(w), None, ptr(y), None, None, *geo, stream())
        with pytest.raises(RuntimeError):
            call('dmy_dwconv_fwd_actbn', 1, ptr(x), ptr(w), None, ptr(y), *geo, None, None, 4, None, 0, stream())
        with pytest.raises(RuntimeError):
            call('dmy_dwconv_dgrad', 1, ptr(x), ptr(w), ptr(y), 0, *geo, stream())
        with pytest.raises(RuntimeError):
            call('dmy_dwconv_wgrad', 1, ptr(x), ptr(x), ptr(part), *geo, stream())
    with pytest.raises(RuntimeError):
        call('dmy_dwconv_fwd_actbn', 1, ptr(x), ptr(w), None, ptr(y), 1, 12, 12, 16, 16, 7, 7, 1, 3, 12, 12, 16, None, None,
             4, None, 0, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all())
