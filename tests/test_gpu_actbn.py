"""GPU: the four act-then-BN passes of csrc/convmix.hip (conv -> GELU -> BatchNorm2d, models/cspcm.py:28-37) through
the C ABI against float64 on the same storage-rounded operands, (M, C) = (35, 8), (70, 24), (257, 64), bf16 and fp32,
every tensor read / written through its own pixel stride inside a guard band.  z ~ N(0, 1.5) spans GELU's curved region.

Bounds (the method of tests/test_gpu_eltwise.py): an elementwise result is a few fp32 operations on an erf / exp that is
accurate to a few ulp, then one storage rounding: |err| <= ulp(T) / 2 * |ref| + 2^-19 * mag, mag the sum of the absolute
values of the terms as common.h evaluates them (GELU = 0.5 u (1 + erf), GELU' = 0.5 (1 + erf) + u phi(u): 1 + erf
cancels for u << 0 and GELU' has a root at u = -0.75, so the terms are 0.5, 0.5 erf and u phi).  A column sum of M terms passes through under M + 16 fp32 additions on terms each accurate to
2^-21: |err| <= (M + 16) * 2^-24 * sum |t| + 2^-20 * sum |t|."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_dw7 import _guarded, _guard_ok

pytestmark = pytest.mark.gpu

GELU = 4
SHAPES = [(35, 8), (70, 24), (257, 64)]
CASES = [(dt, i) for dt in (torch.float32, torch.bfloat16) for i in range(3)]
IDS = [f'{str(dt)[6:]}-{SHAPES[i][0]}x{SHAPES[i][1]}' for dt, i in CASES]
SENT = 7.0


def _strided(t, ps):
    """(M, C) -> (flat, (M, ps) buffer in a guard band, its [:, :C] view holding t)"""
    M, C = t.shape
    flat, buf = _guarded((M, ps), t.dtype)
    buf[:, :C].copy_(t)
    return flat, buf, buf[:, :C]


def _rest(flat, buf, C):
    return _guard_ok(flat) and bool((buf[:, C:] == SENT).all())


def _inputs(dtype, i):
    M, C = SHAPES[i]
    g = torch.Generator().manual_seed(40 + i)
    z = (torch.randn(M, C, generator=g) * 1.5).to(dtype).cuda()
    dy = torch.randn(M, C, generator=g).to(dtype).cuda()
    res = torch.randn(M, C, generator=g).to(dtype).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    return M, C, z, dy, res, gamma, beta


def _dgelu(u):
    return 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * torch.pi) ** 0.5


@pytest.mark.parametrize('dtype,i', CASES, ids=IDS)
def test_actbn_passes_against_float64(dtype, i):
    from dmayolo.functional import call, ptr, stream
    M, C, z, dy, res, gamma, beta = _inputs(dtype, i)
    dt = 1 if dtype == torch.bfloat16 else 0
    vw = 8 if dt else 4
    zps, dps, rps, yps, dzps = C + vw, C + 2 * vw, C + 3 * vw, C + 4 * vw, C + 5 * vw  # distinct pixel strides
    zf, zb, zv = _strided(z, zps)
    gf, gb, gv = _strided(dy, dps)
    rf, rb, rv = _strided(res, rps)
    P = call('dmy_bn_partial_rows', M)
    half_ulp = 2.0 ** -8 if dt else 2.0 ** -24
    zd, dyd = z.double(), dy.double()
    a = F.gelu(zd)
    csum = (M + 16) * 2.0 ** -24 + 2.0 ** -20

    def run():
        out = {}
        ps, pq = torch.full((P, C), float('nan'), device='cuda'), torch.full((P, C), float('nan'), device='cuda')
        call('dmy_actbn_stats', dt, ptr(zv), zps, GELU, M, C, ptr(ps), ptr(pq), stream())
        mean, invstd, scale, shift = (torch.empty(C, device='cuda') for _ in range(4))
        call('dmy_bn_finalize', ptr(ps), ptr(pq), P, C, float(M), ptr(gamma), ptr(beta), None, None, None, 0.0, 1e-3, 0,
             ptr(mean), ptr(invstd), ptr(scale), ptr(shift), stream())
        yf, yb, yv = _strided(torch.full_like(z, float('nan')), yps)
        call('dmy_actbn_fwd', dt, ptr(zv), zps, GELU, ptr(scale), ptr(shift), ptr(rv), rps, ptr(yv), yps, M, C, stream())
        pdb, pdg = torch.full((P, C), float('nan'), device='cuda'), torch.full((P, C), float('nan'), device='cuda')
        call('dmy_actbn_bwd_reduce', dt, ptr(zv), zps, ptr(gv), dps, ptr(mean), ptr(invstd), GELU, M, C, ptr(pdb),
             ptr(pdg), stream())
        dgamma, dbeta, ca, cb, cc = (torch.empty(C, device='cuda') for _ in range(5))
        call('dmy_bn_bwd_finalize', ptr(pdb), ptr(pdg), P, C, float(M), ptr(gamma), ptr(invstd), ptr(dgamma), ptr(dbeta),
             ptr(ca), ptr(cb), ptr(cc), stream())
        df, dbuf, dzv = _strided(torch.full_like(z, float('nan')), dzps)
        pdz = torch.full((P, C), float('nan'), device='cuda')
        call('dmy_actbn_bwd_apply', dt, ptr(zv), zps, ptr(gv), dps, ptr(mean), ptr(invstd), GELU, ptr(ca), ptr(cb),
             ptr(cc), ptr(dzv), dzps, M, C, ptr(pdz), stream())
        dbias = torch.empty(C, device='cuda')
        call('dmy_reduce_rows', ptr(pdz), P, C, ptr(dbias), 0, stream())
        # eval mode: ca = scale, cb = cc = 0, no sums
        zero = torch.zeros(C, device='cuda')
        ef, ebuf, ezv = _strided(torch.full_like(z, float('nan')), dzps)
        call('dmy_actbn_bwd_apply', dt, ptr(zv), zps, ptr(gv), dps, ptr(mean), ptr(invstd), GELU, ptr(scale), ptr(zero),
             ptr(zero), ptr(ezv), dzps, M, C, None, stream())
        torch.cuda.synchronize()
        assert _rest(yf, yb, C) and _rest(df, dbuf, C) and _rest(ef, ebuf, C)
        assert _rest(zf, zb, C) and _rest(gf, gb, C) and _rest(rf, rb, C)
        for k, v in dict(ps=ps, pq=pq, pdb=pdb, pdg=pdg, pdz=pdz).items():
            assert torch.isfinite(v).all(), f'{k}: every partial row must be written'
        out.update(ps=ps, pq=pq, mean=mean, invstd=invstd, scale=scale, shift=shift, y=yv.clone(), pdb=pdb, pdg=pdg,
                   dgamma=dgamma, dbeta=dbeta, dz=dzv.clone(), pdz=pdz, dbias=dbias, edz=ezv.clone())
        return out

    r, r2 = run(), run()
    for k in r:
        assert torch.equal(r[k], r2[k]), f'{k} differs between two runs'
    # statistics of a
    s1, s2 = a.sum(0), (a * a).sum(0)
    assert bool(((r['ps'].double().sum(0) - s1).abs() <= csum * a.abs().sum(0)).all())
    assert bool(((r['pq'].double().sum(0) - s2).abs() <= 2 * csum * s2).all())
    mu = s1 / M
    var = (s2 / M - mu * mu).clamp_min(0)
    # the kernels' own mean / invstd (fp32, from the kernels' sums) feed the later passes: the references use them too
    mean, invstd, scale, shift = (r[k].double() for k in ('mean', 'invstd', 'scale', 'shift'))
    assert float((mean - mu).abs().max()) <= 1e-5 and float((invstd * (var + 1e-3).sqrt() - 1).abs().max()) <= 1e-4
    # forward
    want = a * scale + shift + res.double()
    amag = 0.5 * zd.abs() * (1 + torch.erf(zd / 2 ** 0.5).abs())  # GELU = 0.5 u (1 + erf): the same cancellation
    bound = half_ulp * want.abs() + 2.0 ** -19 * ((amag * scale).abs() + shift.abs() + res.double().abs())
    wy = float(((r['y'].double() - want).abs() / bound).max())
    # backward reduce
    ahat = (a - mean) * invstd
    eb = float(((r['pdb'].double().sum(0) - dyd.sum(0)).abs() / (csum * dyd.abs().sum(0))).max())
    eg = float(((r['pdg'].double().sum(0) - (dyd * ahat).sum(0)).abs() / (csum * (dyd * ahat).abs().sum(0) +
                                                                         2.0 ** -19 * dyd.abs().sum(0))).max())
    assert torch.equal(r['dbeta'], r['pdb'].double().sum(0).float()) or float(
        (r['dbeta'].double() - dyd.sum(0)).abs().max()) <= float((csum * dyd.abs().sum(0)).max())
    # backward apply, with the kernels' own coefficient sums
    sdy, sdg = r['dbeta'].double(), r['dgamma'].double()
    k = gamma.double() * invstd
    da = k * (dyd - sdy / M - ahat * sdg / M)
    wdz = _dgelu(zd) * da
    # GELU' as common.h evaluates it, 0.5 * (1 + erf(u / sqrt 2)) + u phi(u): the terms 0.5, 0.5 erf and u phi cancel
    # (1 + erf for u << 0, the root at u = -0.75), so its fp32 error is relative to the sum of their absolute values
    gmag = 0.5 + 0.5 * torch.erf(zd / 2 ** 0.5).abs() + zd.abs() * torch.exp(-0.5 * zd * zd) / (2 * torch.pi) ** 0.5
    mag = gmag * k.abs() * (dyd.abs() + sdy.abs() / M + ahat.abs() * sdg.abs() / M)
    bdz = half_ulp * wdz.abs() + 2.0 ** -19 * mag
    ez = float(((r['dz'].double() - wdz).abs() / bdz).max())
    wedz = _dgelu(zd) * scale * dyd
    ee = float(((r['edz'].double() - wedz).abs() / (half_ulp * wedz.abs() + 2.0 ** -19 * gmag * (scale * dyd).abs() + 1e-30)).max())
    # the bias gradient: the column sums of dz before the storage rounding
    ed = float(((r['dbias'].double() - wdz.sum(0)).abs() / (csum * mag.sum(0))).max())
    assert torch.equal(r['dbias'], r['pdz'].double().sum(0).float())
    print(f'{dtype} {M}x{C}: err / bound  fwd {wy:.3g}  sum dy {eb:.3g}  sum dy.ahat {eg:.3g}  dz {ez:.3g}  '
          f'eval dz {ee:.3g}  sum dz {ed:.3g}')
    assert max(wy, eb, eg, ez, ee, ed) <= 1.0, (wy, eb, eg, ez, ee, ed)
    assert float(r['dbias'].abs().max()) > 1e-3  # not zero behind an activation


def test_actbn_rejects_what_is_not_whole_vectors():
    from dmayolo.functional import call, ptr, stream
    z = torch.zeros(8, 16, dtype=torch.bfloat16, device='cuda')
    y = torch.full((8, 16), float('nan'), dtype=torch.bfloat16, device='cuda')
    p = torch.full((1, 16), float('nan'), device='cuda')
    one = torch.ones(16, device='cuda')
    with pytest.raises(RuntimeError):
        call('dmy_actbn_stats', 1, ptr(z), 12, GELU, 8, 12, ptr(p), ptr(p), stream())
    with pytest.raises(RuntimeError):
        call('dmy_actbn_fwd', 1, ptr(z), 16, GELU, ptr(one), ptr(one), None, 0, ptr(y), 12, 8, 16, stream())
    with pytest.raises(RuntimeError):
        call('dmy_actbn_bwd_apply', 1, ptr(z), 16, ptr(z), 16, ptr(one), ptr(one), GELU, ptr(one), ptr(one), ptr(one),
             ptr(y[:, 4:]), 16, 8, 8, None, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(p).all())
