"""GPU, one process, through the C ABI: the SyncBatchNorm slab kernels of csrc/bn.hip (dmy_bn_sync_pack /
dmy_bn_sync_finalize / dmy_bn_sync_bwd_finalize) against dmy_bn_finalize / dmy_bn_bwd_finalize over the whole batch and
against float64 (tests/syncbn_ref.py).

Data: M = 600 partial rows of C channels, C in {4, 24, 520} (520 channels: more than the 256 a finalize block covers, and
the third block is ragged), row m holding (x, x * x) of one pixel, so a part of n rows has n pixels.  The rows are split
into R in {1, 2, 3} consecutive parts, [600], [1, 599] and [37, 5, 558]: a part of a single row, and a part of more than
256 rows (more than one row per thread of the pack).  Each "rank" packs its part into its own NaN-filled slab; the sum
of the R slabs stands in for the all-reduce.

Bounds.  tests/test_gpu_actbn.py holds dmy_bn_finalize to |mean - mu| <= 1e-5 and |invstd * sqrt(var + eps) - 1| <=
1e-4 against float64: the same two bounds hold here.  It has none for scale / shift / the running statistics / the
backward coefficients, so each case measures dmy_bn_finalize's (dmy_bn_bwd_finalize's) own largest absolute error against
float64 on the same data, e, and allows the slab path 2e against float64, hence 3e against the whole-batch kernel.
Measured e on the MI355X: DESIGN.md §5 (SyncBatchNorm)."""
import numpy as np
import pytest
import torch

import syncbn_ref as ref

pytestmark = pytest.mark.gpu

M = 600
SPLITS = {1: [600], 2: [1, 599], 3: [37, 5, 558]}
EPS, MOM = 1e-3, 0.03
CASES = [(C, R) for C in (4, 24) for R in (1, 2, 3)] + [(520, 3)]
FWD = ('mean', 'invstd', 'scale', 'shift', 'rmean', 'rvar')
BWD = ('ca', 'cb', 'cc')


def _data(C):
    g = torch.Generator().manual_seed(100 + C)
    x = torch.randn(M, C, generator=g) * 1.7 + 0.3
    dy = torch.randn(M, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rmean, rvar = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return x, dy, gamma, beta, rmean, rvar


def _pack(pa, pb, lo, hi, slab, R, rank):
    from dmayolo.functional import call, ptr, stream
    a, b = pa[lo:hi].contiguous(), pb[lo:hi].contiguous()
    call('dmy_bn_sync_pack', ptr(a), ptr(b), hi - lo, pa.shape[1], float(hi - lo), ptr(slab), R, rank, stream())


def _exchange(pa, pb, parts):
    """-> (the reduced slab [R][2C + 1], the per-rank slabs): every rank packs into NaN garbage, the sum is the collective"""
    R, C = len(parts), pa.shape[1]
    slabs = []
    for r, (lo, hi) in enumerate(parts):
        s = torch.full((R, 2 * C + 1), float('nan'), dtype=torch.float64, device='cuda')
        _pack(pa, pb, lo, hi, s, R, r)
        slabs.append(s)
    total = slabs[0].clone()
    for s in slabs[1:]:
        total += s
    return total, slabs


def _finalize(C, gamma, beta, rmean, rvar, slab=None, R=0, pa=None, pb=None):
    """dmy_bn_sync_finalize over the slab, or dmy_bn_finalize over all rows -> dict of the six outputs and nbt"""
    from dmayolo.functional import call, ptr, stream
    o = {k: torch.full((C,), float('nan'), device='cuda') for k in ('mean', 'invstd', 'scale', 'shift')}
    o['rmean'], o['rvar'] = rmean.clone(), rvar.clone()
    o['nbt'] = torch.tensor(41, dtype=torch.int64, device='cuda')
    tail = (ptr(gamma), ptr(beta), ptr(o['rmean']), ptr(o['rvar']), ptr(o['nbt']), MOM, EPS, 1, ptr(o['mean']),
            ptr(o['invstd']), ptr(o['scale']), ptr(o['shift']), stream())
    if slab is not None:
        call('dmy_bn_sync_finalize', ptr(slab), R, C, *tail)
    else:
        call('dmy_bn_finalize', ptr(pa), ptr(pb), pa.shape[0], C, float(pa.shape[0]), *tail)
    return o


def _bwd_finalize(C, gamma, invstd, slab=None, R=0, rank=0, pa=None, pb=None):
    from dmayolo.functional import call, ptr, stream
    o = {k: torch.full((C,), float('nan'), device='cuda') for k in ('dgamma', 'dbeta') + BWD}
    tail = (ptr(gamma), ptr(invstd), ptr(o['dgamma']), ptr(o['dbeta']), ptr(o['ca']), ptr(o['cb']), ptr(o['cc']), stream())
    if slab is not None:
        call('dmy_bn_sync_bwd_finalize', ptr(slab), R, rank, C, *tail)
    else:
        call('dmy_bn_bwd_finalize', ptr(pa), ptr(pb), pa.shape[0], C, float(pa.shape[0]), *tail)
    return o


def _err(t, want):
    return float(np.abs(t.double().cpu().numpy() - want).max())


@pytest.mark.parametrize('C,R', CASES)
def test_forward_slab_against_whole_batch_and_float64(C, R):
    x, dy, gamma, beta, rmean, rvar = (t.cuda() for t in _data(C))
    pa, pb = x, x * x  # the fp32 partial rows a stats pass would hand over: one pixel per row
    parts = ref.split_rows(M, SPLITS[R])
    slab, _ = _exchange(pa, pb, parts)
    got = _finalize(C, gamma, beta, rmean, rvar, slab=slab, R=R)
    slab2, _ = _exchange(pa, pb, parts)
    again = _finalize(C, gamma, beta, rmean, rvar, slab=slab2, R=R)
    whole = _finalize(C, gamma, beta, rmean, rvar, pa=pa, pb=pb)
    torch.cuda.synchronize()
    assert torch.equal(slab, slab2)
    for k in got:
        assert torch.equal(got[k], again[k]), f'{k} differs between two runs'
    assert int(got['nbt']) == int(whole['nbt']) == 42
    if R == 1:
        for k in got:
            assert torch.equal(got[k], whole[k]), f'{k}: one rank must reproduce dmy_bn_finalize bit for bit'
    # float64 over the same fp32 rows (the kernels' input): sums of the parts, merged in rank order
    pan, pbn = pa.double().cpu().numpy(), pb.double().cpu().numpy()
    st = ref.stats_from_sums(*ref.merge([ref.slot(pan[lo:hi], pbn[lo:hi]) for lo, hi in parts]), gamma.cpu().numpy(),
                             beta.cpu().numpy(), EPS)
    run = ref.running(rmean.cpu().numpy(), rvar.cpu().numpy(), st, MOM)
    want = dict(mean=st['mean'], invstd=st['invstd'], scale=st['scale'], shift=st['shift'], rmean=run[0], rvar=run[1])
    e = {k: _err(whole[k], want[k]) for k in FWD}
    print(f'C={C} R={R} dmy_bn_finalize |err| vs float64: ' + ' '.join(f'{k} {e[k]:.3e}' for k in FWD))
    print(f'C={C} R={R} dmy_bn_sync_finalize |err|       : ' + ' '.join(f'{k} {_err(got[k], want[k]):.3e}' for k in FWD))
    assert _err(got['mean'], want['mean']) <= 1e-5
    assert float(np.abs(got['invstd'].double().cpu().numpy() * np.sqrt(st['var'] + EPS) - 1).max()) <= 1e-4
    for k in FWD:
        assert _err(got[k], want[k]) <= 2 * e[k], (k, _err(got[k], want[k]), e[k])
        assert float((got[k].double() - whole[k].double()).abs().max()) <= 3 * e[k], k


@pytest.mark.parametrize('C,R', CASES)
def test_backward_slab_against_whole_batch_and_float64(C, R):
    x, dy, gamma, beta, rmean, rvar = (t.cuda() for t in _data(C))
    invstd = 1.0 / (x.var(0, unbiased=False) + EPS).sqrt()
    xhat = (x - x.mean(0)) * invstd
    pa, pb = dy, dy * xhat  # the reduce pass's partial rows (sum dy, sum dy * xhat), one pixel per row
    parts = ref.split_rows(M, SPLITS[R])
    slab, _ = _exchange(pa, pb, parts)
    got = [_bwd_finalize(C, gamma, invstd, slab=slab, R=R, rank=r) for r in range(R)]
    again = [_bwd_finalize(C, gamma, invstd, slab=slab, R=R, rank=r) for r in range(R)]
    whole = _bwd_finalize(C, gamma, invstd, pa=pa, pb=pb)
    torch.cuda.synchronize()
    for r in range(R):
        for k in got[r]:
            assert torch.equal(got[r][k], again[r][k]), f'{k} differs between two runs'
        for k in BWD:  # the coefficients are the same bits on every rank
            assert torch.equal(got[r][k], got[0][k]), (r, k)
        # dgamma / dbeta: slot `rank`'s own sums, rounded to fp32 once
        assert torch.equal(got[r]['dbeta'], slab[r, :C].float()) and torch.equal(got[r]['dgamma'], slab[r, C:2 * C].float())
    if R == 1:
        for k in whole:
            assert torch.equal(got[0][k], whole[k]), f'{k}: one rank must reproduce dmy_bn_bwd_finalize bit for bit'
    pan, pbn = pa.double().cpu().numpy(), pb.double().cpu().numpy()
    slots = [ref.slot(pan[lo:hi], pbn[lo:hi]) for lo, hi in parts]
    g64, is64 = gamma.double().cpu().numpy(), invstd.double().cpu().numpy()
    want = ref.bwd_from_slots(slots, 0, g64, is64)
    full = ref.bwd_from_slots([ref.slot(pan, pbn)], 0, g64, is64)
    e = {k: _err(whole[k], full[k]) for k in BWD + ('dgamma', 'dbeta')}
    print(f'C={C} R={R} dmy_bn_bwd_finalize |err| vs float64: ' + ' '.join(f'{k} {v:.3e}' for k, v in e.items()))
    for k in BWD:
        assert _err(got[0][k], want[k]) <= 2 * e[k], (k, _err(got[0][k], want[k]), e[k])
        assert float((got[0][k].double() - whole[k].double()).abs().max()) <= 3 * e[k], k
    assert torch.equal(got[0]['ca'], whole['ca'])  # one fp32 product of the inputs: the same bits in both kernels
    # the ranks' parameter gradients sum to the whole batch's: each is float64 rounded to fp32 once (2^-24 relative, and
    # 2^-40 for the order of the float64 sum),
    # against the whole-batch kernel's own error e
    for k, i in (('dbeta', 0), ('dgamma', 1)):
        for r in range(R):
            assert _err(got[r][k], slots[r][i]) <= (2.0 ** -24 + 2.0 ** -40) * float(np.abs(slots[r][i]).max())
        tot = sum(o[k].double().cpu().numpy() for o in got)
        bound = 2 * e[k] + 2.0 ** -24 * sum(np.abs(s[i]) for s in slots)
        assert bool((np.abs(tot - full[k]) <= bound).all()), k


@pytest.mark.parametrize('C', [4, 520])
def test_pack_zeroes_every_other_slot(C):
    """into a NaN-filled slab: slot `rank` holds the float64 column sums and the count, every other slot is +0.0"""
    x = _data(C)[0].cuda()
    pa, pb = x, x * x
    R = 3
    for rank, (lo, hi) in enumerate(ref.split_rows(M, SPLITS[R])):
        slab = torch.full((R, 2 * C + 1), float('nan'), dtype=torch.float64, device='cuda')
        guard = torch.full((R * (2 * C + 1) + 64,), 7.0, dtype=torch.float64, device='cuda')
        inner = guard[32:32 + R * (2 * C + 1)].view(R, 2 * C + 1)
        inner.copy_(slab)
        _pack(pa, pb, lo, hi, inner, R, rank)
        torch.cuda.synchronize()
        assert bool((guard[:32] == 7.0).all()) and bool((guard[-32:] == 7.0).all())
        others = [r for r in range(R) if r != rank]
        assert bool((inner[others] == 0).all()) and not bool(torch.signbit(inner[others]).any())
        assert float(inner[rank, 2 * C]) == hi - lo
        sa, sb, _ = ref.slot(pa[lo:hi].double().cpu().numpy(), pb[lo:hi].double().cpu().numpy())
        np.testing.assert_allclose(inner[rank, :C].cpu().numpy(), sa, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(inner[rank, C:2 * C].cpu().numpy(), sb, rtol=1e-13, atol=1e-13)
