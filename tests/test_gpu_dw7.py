"""GPU: the depthwise 7x7 stride-1 conv with bias (csrc/dwconv.hip, get_dwconv of GnConv, models/common.py:1361-1362)
through the C ABI against float64 torch on the same storage-rounded operands, bf16 and fp32.  The inputs of the three
small shapes are those of tests/golden/dw7.npz (tools/gen_golden_hor.py: the reference module on the CPU), whose recorded
fp32 outputs and gradients must agree with the float64 computation to 1e-5 rel-L2; the fourth shape would not fit a
committed file and is drawn from a seeded generator.

Shapes (N, H, W, C), C0 = 8 (bf16) / 4 (fp32): (2, 5, 6, C0), a map smaller than the filter, every tap a border tap;
(1, 7, 9, 3 C0), a unit count that is no power of two; (2, 16, 20, C0) read from and written to channels [2 C0, 3 C0) of
4 C0-channel buffers; (2, 40, 44, 17 C0), 14 partial rows and a grid stride of several steps per block.

Bounds.
fp32 forward / data-grad / weight-grad: the expression of tests/test_gpu_dwconv.py's fp32 cases, rel-L2 against float64
at most 4x that of torch's own fp32 depthwise conv on the same inputs.
bf16 forward / data-grad, per element: 49 products of bf16 values are exact in fp32, their sum passes through at most 50
fp32 additions (bias included), 50 * 2^-24 < 2^-18 relative to sum |x w| + |b|, then one rounding to bf16, half an ulp
of 8 significand bits, at most 2^-8 relative.  Bound: 2^-8 |ref| + 2^-18 (sum |x w| + |b|).
Reductions (weight-grad taps, bias-grad; both dtypes), per output: a product (exact in bf16 storage, one rounding in fp32)
and a chain of additions -- 4 per strip and at most ceil(55 / 14) = 4 strips per thread, 6 shuffle levels, 3 across the
waves, 14 partial rows: 39 in the largest case here -- under 2^6 roundings of 2^-24 each relative to sum |t|.  Bound:
2^-18 * sum |t| with t computed in float64.
Every output lies in a buffer with a guard band on both sides (and, for the slice case, the other channels) that must
stay untouched, and a second run must be bit-identical.
The BN-statistics forward and the fused inference epilogue are the k = 3 / 5 code at K = 7; their two tests repeat the
checks and bounds of tests/test_gpu_dwconv.py on the (1, 7, 9, 3 C0) and slice shapes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
K, P = 7, 3
GUARD, SENTINEL = 64, 7.0


def _shapes(dtype):
    c0 = 8 if dtype == torch.bfloat16 else 4
    return [(2, 5, 6, c0, c0, 0), (1, 7, 9, 3 * c0, 3 * c0, 0), (2, 16, 20, c0, 4 * c0, 2 * c0),
            (2, 40, 44, 17 * c0, 17 * c0, 0)]


CASES = [(dt, i) for dt in (torch.float32, torch.bfloat16) for i in range(4)]
IDS = [f'{str(dt)[6:]}-s{i}' for dt, i in CASES]


def _guarded(shape, dtype, fill=SENTINEL):
    """-> (flat buffer, view of `shape` in its middle): GUARD sentinel elements on either side (16-byte multiples)"""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guard_ok(flat):
    return bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all())


def _nhwc(t, Ct, c0):
    """t (N, C, H, W) -> (flat, buffer (N, Ct, H, W) NHWC inside a guard band, its channel slice holding t); the other
    channels hold the sentinel"""
    N, C, H, W = t.shape
    flat, store = _guarded((N, H, W, Ct), t.dtype)
    buf = store.permute(0, 3, 1, 2)
    v = buf[:, c0:c0 + C]
    v.copy_(t)
    return flat, buf, v


def _rest_ok(flat, buf, C, c0):
    rest = torch.cat([buf[:, :c0], buf[:, c0 + C:]], 1)
    return _guard_ok(flat) and bool((rest == SENTINEL).all())


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


_CACHE = {}
_GOLD = []


def _gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dw7.npz')))
    return _GOLD[0]


def _case(dtype, i):
    """inputs (storage-rounded, on the GPU) and the float64 references of one shape, computed once"""
    key = (dtype, i)
    if key not in _CACHE:
        N, H, W, C, Ct, c0 = _shapes(dtype)[i]
        c0k, gold = 8 if dtype == torch.bfloat16 else 4, None
        if i < 3:
            gold = {k: torch.from_numpy(_gold()[f'{c0k}.{i}.{k}']) for k in ('x', 'w', 'b', 'dz', 'y', 'dx', 'dw', 'db')}
            x, w, b, dz = gold['x'], gold['w'], gold['b'], gold['dz']
            assert tuple(x.shape) == (N, C, H, W)
        else:
            g = torch.Generator().manual_seed(700 + i)
            x, w = torch.randn(N, C, H, W, generator=g), torch.randn(C, 1, K, K, generator=g) / K
            b, dz = torch.randn(C, generator=g), torch.randn(N, C, H, W, generator=g)
        x, w, b, dz = x.to(dtype).cuda(), w.cuda(), b.cuda(), dz.to(dtype).cuda()
        ws = w.to(dtype)  # the filter operand is in the storage dtype
        xd, wd, zd = x.double(), ws.double(), dz.double()
        ref = dict(
            y=F.conv2d(xd, wd, b.double(), padding=P, groups=C),
            ymag=F.conv2d(xd.abs(), wd.abs(), b.double().abs(), padding=P, groups=C),
            dx=torch.nn.grad.conv2d_input((N, C, H, W), wd, zd, padding=P, groups=C),
            dxmag=torch.nn.grad.conv2d_input((N, C, H, W), wd.abs(), zd.abs(), padding=P, groups=C),
            dw=torch.nn.grad.conv2d_weight(xd, (C, 1, K, K), zd, padding=P, groups=C),
            dwmag=torch.nn.grad.conv2d_weight(xd.abs(), (C, 1, K, K), zd.abs(), padding=P, groups=C),
            db=zd.sum((0, 2, 3)), dbmag=zd.abs().sum((0, 2, 3)))
        t32 = None
        if gold is not None and dtype == torch.float32:  # the recorded reference and the float64 computation agree
            for k in ('y', 'dx', 'dw', 'db'):
                assert _rel(gold[k].cuda(), ref[k]) < 1e-5, k
        if dtype == torch.float32:
            t32 = dict(y=F.conv2d(x, w, b, padding=P, groups=C),
                       dx=torch.nn.grad.conv2d_input((N, C, H, W), w, dz, padding=P, groups=C),
                       dw=torch.nn.grad.conv2d_weight(x, (C, 1, K, K), dz, padding=P, groups=C))
        _CACHE[key] = (x, w, b, dz, ref, t32)
    return _CACHE[key]


def _wop(w, dtype):
    from dmayolo.functional import prep_weight
    return prep_weight(w, dtype, True)[1]  # the IHWO copy of (C, 1, k, k) == [k][k][C]


def _check_map(name, got, ref, mag, t32, dtype):
    if dtype == torch.float32:
        own, err = _rel(t32, ref), _rel(got, ref)
        print(f'fp32 {name}: torch {own:.2e} kernel {err:.2e}')
        assert err <= 4 * own, (name, err, own)
    else:
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -18 * mag
        worst = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
        print(f'bf16 {name}: max err / bound {worst:.3g}')
        assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw7_fwd_bias(dtype, i):
    from dmayolo.functional import call, ptr, stream
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    x, w, b, _, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    xf, xb, xv = _nhwc(x, Ct, c0)
    wd = _wop(w, dtype)
    assert call('dmy_dwconv_ok', dt, ptr(xv), ptr(wd), ptr(xv), N, H, W, C, C, C, Ct, K, K, 1, P, H, W, Ct) == 1
    outs = []
    for run in range(2):
        yf, yb, yv = _nhwc(torch.full_like(x, float('nan')), Ct, c0)
        call('dmy_dwconv_fwd_act', dt, ptr(xv), ptr(wd), ptr(b), ptr(yv), N, H, W, C, Ct, K, K, 1, P, H, W, Ct, None, None,
             0, None, 0, stream())
        torch.cuda.synchronize()
        assert _rest_ok(yf, yb, C, c0) and _rest_ok(xf, xb, C, c0)
        assert torch.isfinite(yv).all()
        outs.append(yv.clone())
    assert torch.equal(outs[0], outs[1])
    _check_map('fwd', outs[0], ref['y'], ref['ymag'], t32 and t32['y'], dtype)


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw7_dgrad(dtype, i):
    from dmayolo.functional import call, ptr, stream
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    _, w, _, dz, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    zf, zb, zv = _nhwc(dz, Ct, c0)
    wd = _wop(w, dtype)
    outs = []
    for run in range(2):
        df, db_, dv = _nhwc(torch.full_like(dz, float('nan')), Ct, c0)
        call('dmy_dwconv_dgrad', dt, ptr(zv), ptr(wd), ptr(dv), 0, N, H, W, C, Ct, K, K, 1, P, H, W, Ct, stream())
        torch.cuda.synchronize()
        assert _rest_ok(df, db_, C, c0) and _rest_ok(zf, zb, C, c0)
        assert torch.isfinite(dv).all()
        outs.append(dv.clone())
    assert torch.equal(outs[0], outs[1])
    _check_map('dgrad', outs[0], ref['dx'], ref['dxmag'], t32 and t32['dx'], dtype)


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_dw7_wgrad_and_bias_grad(dtype, i):
    from dmayolo.functional import call, ptr, stream
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    x, _, _, dz, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    _, _, xv = _nhwc(x, Ct, c0)
    _, _, zv = _nhwc(dz, Ct, c0)
    rows = call('dmy_dwconv_wgrad_rows', N * H * W, C)
    outs = []
    for run in range(2):
        pf, part = _guarded((rows, (K * K + 1) * C), torch.float32)
        part.fill_(float('nan'))
        wf, dw = _guarded((C, 1, K, K), torch.float32)
        bf, db = _guarded((C,), torch.float32)
        call('dmy_dwconv_wgrad_bias', dt, ptr(xv), ptr(zv), ptr(part), N, H, W, C, Ct, K, K, 1, P, H, W, Ct, stream())
        call('dmy_dwconv_wgrad_bias_finalize', ptr(part), rows, C, K, K, ptr(dw), 0, ptr(db), 0, stream())
        torch.cuda.synchronize()
        assert _guard_ok(pf) and _guard_ok(wf) and _guard_ok(bf)
        assert torch.isfinite(part).all(), 'every partial row must be written'
        outs.append((dw.clone(), db.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dw, db = outs[0]
    ew = float(((dw.double() - ref['dw']).abs() / (2.0 ** -18 * ref['dwmag']).clamp_min(1e-300)).max())
    eb = float(((db.double() - ref['db']).abs() / (2.0 ** -18 * ref['dbmag']).clamp_min(1e-300)).max())
    print(f'{dtype} wgrad max err / bound {ew:.3g}, bias-grad {eb:.3g}, rows {rows}')
    assert ew <= 1.0 and eb <= 1.0, (ew, eb)
    if dtype == torch.float32:
        own, err = _rel(t32['dw'], ref['dw']), _rel(dw, ref['dw'])
        assert err <= 4 * own, (err, own)
    # the plain weight-grad entry writes the same filter gradient from rows without the bias share, and both finalizes
    # accumulate
    part2 = torch.full((rows, K * K * C), float('nan'), device='cuda')
    dw2 = torch.ones(C, 1, K, K, device='cuda')
    call('dmy_dwconv_wgrad', dt, ptr(xv), ptr(zv), ptr(part2), N, H, W, C, Ct, K, K, 1, P, H, W, Ct, stream())
    call('dmy_dwconv_wgrad_finalize', ptr(part2), rows, C, K, K, ptr(dw2), 1, stream())
    dw3, db3 = torch.ones(C, 1, K, K, device='cuda'), torch.ones(C, device='cuda')
    call('dmy_dwconv_wgrad_bias_finalize', ptr(part), rows, C, K, K, ptr(dw3), 1, ptr(db3), 1, stream())
    torch.cuda.synchronize()
    assert torch.equal(dw2, 1 + dw) and torch.equal(dw3, 1 + dw) and torch.equal(db3, 1 + db)


class _Owner(torch.nn.Module):
    """stands in for the nn.Conv2d(dim, dim, 7, padding=3, groups=dim) that owns the ConvSpec"""

    def __init__(self, C):
        super().__init__()
        self.groups = C


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_dw7_autograd_bias_path(dtype):
    """conv_bn_act on a biased 7x7 depthwise layer: the forward (with and without grad) and the three gradients of one
    backward equal the C-ABI launches bit for bit (the bias gradient comes out of the weight-grad launch), and the
    forward holds the bound of test_dw7_fwd_bias"""
    from dmayolo.functional import call, ptr, stream, conv_bn_act, spec_for, ACT_NONE
    i = 1
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    x, w, b, dz, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    owner = _Owner(C)
    xi = x.contiguous(memory_format=CL).requires_grad_(True)
    wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = conv_bn_act(xi, wp, bp, None, 1, P, ACT_NONE, spec=spec_for(owner, 1, P, ACT_NONE, None))
    y.backward(dz.contiguous(memory_format=CL))
    torch.cuda.synchronize()
    wd = _wop(w, dtype)
    xv, zv = x.contiguous(memory_format=CL), dz.contiguous(memory_format=CL)
    y2, dx2 = torch.empty_like(xv), torch.empty_like(xv)
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(b), ptr(y2), None, None, N, H, W, C, C, K, K, 1, P, H, W, C, stream())
    call('dmy_dwconv_dgrad', dt, ptr(zv), ptr(wd), ptr(dx2), 0, N, H, W, C, C, K, K, 1, P, H, W, C, stream())
    rows = call('dmy_dwconv_wgrad_rows', N * H * W, C)
    part = torch.empty(rows, (K * K + 1) * C, device='cuda')
    dw2, db2 = torch.empty(C, 1, K, K, device='cuda'), torch.empty(C, device='cuda')
    call('dmy_dwconv_wgrad_bias', dt, ptr(xv), ptr(zv), ptr(part), N, H, W, C, C, K, K, 1, P, H, W, C, stream())
    call('dmy_dwconv_wgrad_bias_finalize', ptr(part), rows, C, K, K, ptr(dw2), 0, ptr(db2), 0, stream())
    torch.cuda.synchronize()
    _check_map('autograd fwd', y.detach(), ref['y'], ref['ymag'], t32 and t32['y'], dtype)
    assert torch.equal(y.detach(), y2)
    assert torch.equal(xi.grad, dx2)
    assert torch.equal(wp.grad, dw2) and torch.equal(bp.grad, db2)
    with torch.no_grad():
        ye = conv_bn_act(xi, wp, bp, None, 1, P, ACT_NONE, spec=spec_for(owner, 1, P, ACT_NONE, None))
    assert torch.equal(ye, y2)


def test_dw7_unsupported_launches_nothing():
    """7x7 with stride 2, and the bias weight-grad for any other filter size: the query says 0 / the entries return -1
    (call() raises) and write nothing"""
    from dmayolo.functional import call, ptr, stream
    x = torch.zeros(1, 8, 8, 8, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)
    y = torch.full((1, 8, 4, 4), float('nan'), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=CL)
    w = torch.zeros(49, 8, dtype=torch.bfloat16, device='cuda')
    assert call('dmy_dwconv_ok', 1, ptr(x), ptr(w), ptr(y), 1, 8, 8, 8, 8, 8, 8, 7, 7, 2, 3, 4, 4, 8) == 0
    with pytest.raises(RuntimeError):
        call('dmy_dwconv_fwd_act', 1, ptr(x), ptr(w), None, ptr(y), 1, 8, 8, 8, 8, 7, 7, 2, 3, 4, 4, 8, None, None, 0, None,
             0, stream())
    part = torch.full((1, 10 * 8), float('nan'), device='cuda')
    with pytest.raises(RuntimeError):
        call('dmy_dwconv_wgrad_bias', 1, ptr(x), ptr(x), ptr(part), 1, 8, 8, 8, 8, 3, 3, 1, 1, 8, 8, 8, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('i', [1, 2])
def test_dw7_fwd_bn_partial_sums(dtype, i):
    """the training forward of a 7x7 DWConv with BN: z and the per-row sums of the values as stored"""
    from dmayolo.functional import call, ptr, stream
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    x, w, b, _, ref, t32 = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    _, _, xv = _nhwc(x, Ct, c0)
    zf, zb, zv = _nhwc(torch.full_like(x, float('nan')), Ct, c0)
    M = N * H * W
    rows = call('dmy_dwconv_fwd_rows', M, C)
    pf, ps = _guarded((rows, C), torch.float32)
    qf, pq = _guarded((rows, C), torch.float32)
    ps.fill_(float('nan'))
    pq.fill_(float('nan'))
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(_wop(w, dtype)), ptr(b), ptr(zv), ptr(ps), ptr(pq), N, H, W, C, Ct, K, K, 1, P,
         H, W, Ct, stream())
    torch.cuda.synchronize()
    assert _rest_ok(zf, zb, C, c0) and _guard_ok(pf) and _guard_ok(qf)
    assert torch.isfinite(ps).all() and torch.isfinite(pq).all(), 'every partial row must be written'
    _check_map('fwd (stats)', zv, ref['y'], ref['ymag'], t32 and t32['y'], dtype)
    stored = zv.double()  # the sums are of the values as stored (include/dmayolo.h)
    s1, s2 = stored.sum((0, 2, 3)), (stored ** 2).sum((0, 2, 3))
    e1, e2 = _rel(ps.sum(0), s1), _rel(pq.sum(0), s2)
    print(f'{dtype} psum {e1:.2e} psq {e2:.2e} rows {rows}')
    assert e1 < 1e-3 or float((ps.sum(0).double() - s1).abs().max()) < 1e-2 * M ** 0.5
    assert e2 < 1e-3


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_dw7_fwd_act_equals_two_passes(dtype):
    """dmy_dwconv_fwd_act == dmy_dwconv_fwd + dmy_bn_act_fwd to one storage rounding at K = 7: bias, scale / shift, SiLU
    and a residual on channel slices (the check of tests/test_gpu_dwconv.py's k = 3 / 5 cases)"""
    from dmayolo.functional import call, ptr, stream, ACT_SILU
    i = 2
    N, H, W, C, Ct, c0 = _shapes(dtype)[i]
    x, w, b, dz, _, _ = _case(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    g = torch.Generator().manual_seed(9)
    scale, shift = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    wd = _wop(w, dtype)
    _, _, xv = _nhwc(x, Ct, c0)
    _, _, rv = _nhwc(dz, Ct, c0)  # residual
    yf, yb, yv = _nhwc(torch.zeros_like(dz), Ct, c0)
    _, _, zv = _nhwc(torch.zeros_like(dz), Ct, c0)
    _, _, y2 = _nhwc(torch.zeros_like(dz), Ct, c0)
    call('dmy_dwconv_fwd_act', dt, ptr(xv), ptr(wd), ptr(b), ptr(yv), N, H, W, C, Ct, K, K, 1, P, H, W, Ct, ptr(scale),
         ptr(shift), ACT_SILU, ptr(rv), Ct, stream())
    call('dmy_dwconv_fwd', dt, ptr(xv), ptr(wd), ptr(b), ptr(zv), None, None, N, H, W, C, Ct, K, K, 1, P, H, W, Ct, stream())
    call('dmy_bn_act_fwd', dt, ptr(zv), Ct, ptr(scale), ptr(shift), ACT_SILU, ptr(rv), Ct, ptr(y2), Ct, N * H * W, C,
         stream())
    torch.cuda.synchronize()
    assert _rest_ok(yf, yb, C, c0)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22
    u = (zv.float() * scale.view(1, -1, 1, 1)).abs() + shift.view(1, -1, 1, 1).abs()
    mag = 2.1 * u + rv.float().abs()
    a, c = yv.float(), y2.float()
    assert bool(((a - c).abs() <= ulp * mag).all()), float(((a - c).abs() / mag.clamp_min(1e-30)).max())
