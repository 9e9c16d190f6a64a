"""Kernel-level parity of the BatchNorm streaming entries of csrc/bn.hip against an fp64 restatement written from the
formulas:

  dmy_bn_stats       partial rows of sum z and sum z^2
  dmy_bn_act_fwd     y = act(z * scale + shift) (+ res)
  dmy_bn_bwd_reduce  partial rows of sum du and sum du * (z - mean) * invstd, du = dy * act'(z * scale + shift)
  dmy_bn_bwd_apply   dz = ca * du + cb + cc * (z - mean) * invstd

Each runs in its 16-byte-vector form and in its scalar form (tests/test_gpu_eltwise.py's LAYOUTS: channel counts that
are / are not a vector multiple, a slice of a wider buffer at an aligned / unaligned channel offset), in both storage
types, at M = 7 rows and at M = 1500, where both forms write more than one partial row.

Bounds, per element and derived (eltwise_ref.bound, printed by `check` before it asserts).  u = z * scale + shift is two
fp32 roundings of |z scale| + |shift| (`uabs`).  Forward: that error through an activation of slope at most 1.5
(Hardswish at u = 3), the activation's own few operations, the residual add, the project's fp32 tolerance where sigmoid
/ erf are evaluated, one rounding to the storage type.  du: |dy| times (the error of u through a second derivative of at
most 1, four operations of act', the same tolerance) plus the product's rounding: `edu`.  A column sum of M terms adds
M * 2^-24 * sum |term| to the summed errors of its terms; the second reduce's terms carry three more roundings.  The
apply is evaluated as ca * du + (cb - cc invstd mean) + (cc invstd) * z by the vector form, so its terms are those."""
import pytest
import torch

import eltwise_ref as R
from test_gpu_eltwise import DTYPES, F32, FILL, LAYOUTS, _lib, check, dcode, gen_for, randn, slab, untouched

pytestmark = pytest.mark.gpu

ROWS = [7, 1500]


def coefs(C, gen, kinds):
    """per-channel fp32 vectors, 'p' in [0.5, 1.5) (a scale, an invstd) or 's' signed -> (fp64 CPU copies, device tensors)"""
    cpu = [torch.rand(C, generator=gen) + 0.5 if k == 'p' else torch.randn(C, generator=gen) * 0.3 for k in kinds]
    return [c.double() for c in cpu], [c.cuda() for c in cpu]


def partial_rows(call, ptr, dtype, z, zps, dy, dps, M, C):
    return call('dmy_bn_reduce_rows', dcode(dtype), ptr(z), zps, ptr(dy) if dy is not None else None, dps, M, C)


def expect_vector(C, Ct, off, dtype):
    VW = 8 if dtype != F32 else 4
    return C % VW == 0 and Ct % VW == 0 and off % VW == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,Ct,off', LAYOUTS)
@pytest.mark.parametrize('M', ROWS)
def test_bn_stats(M, C, Ct, off, dtype):
    call, ptr, stream = _lib()
    gen = gen_for(M, C, Ct, off)
    zc = randn((M, C), gen, dtype)
    zbuf, z = slab(zc, Ct, off)
    P = partial_rows(call, ptr, dtype, z, Ct, None, 0, M, C)
    # the vector form writes one row per 256 / (C / VW) * 8 pixels (512 .. 1024 here), the scalar form one per 256
    assert (P > 1) == (M == 1500) and (expect_vector(C, Ct, off, dtype) or P == -(-M // 256))
    ps, pq = torch.full((P, C), float('nan'), device='cuda'), torch.full((P, C), float('nan'), device='cuda')
    call('dmy_bn_stats', dcode(dtype), ptr(z), Ct, M, C, ptr(ps), ptr(pq), stream())
    zd = zc.double()
    check('bn_stats_sum', ps.double().sum(0), zd.sum(0), zd.abs().sum(0), M, F32)
    check('bn_stats_sq', pq.double().sum(0), (zd * zd).sum(0), (zd * zd).sum(0), M + 1, F32)
    assert untouched(zbuf, off, C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,Ct,off', LAYOUTS)
@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_SILU, R.ACT_HARDSWISH, R.ACT_GELU, R.ACT_LEAKY])
def test_bn_act_fwd(act, M, C, Ct, off, dtype):
    call, ptr, stream = _lib()
    gen = gen_for(M, C, Ct, off, act)
    zc, rc = randn((M, C), gen, dtype, 1.5), randn((M, C), gen, dtype)
    (sc, sh), (scale, shift) = coefs(C, gen, 'ps')
    zbuf, z = slab(zc, Ct, off)
    rbuf, res = slab(rc, Ct, off)
    u, uabs = zc.double() * sc + sh, (zc.double() * sc).abs() + sh.abs()
    yr, ya = R.act(act, u)
    for with_res in (False, True):
        ybuf, y = slab(torch.zeros(M, C, dtype=dtype), Ct, off)
        call('dmy_bn_act_fwd', dcode(dtype), ptr(z), Ct, ptr(scale), ptr(shift), act, ptr(res) if with_res else None,
             Ct if with_res else 0, ptr(y), Ct, M, C, stream())
        r = rc.double() * with_res
        check(f'bn_act_fwd_act{act}_res{int(with_res)}', y, yr + r, ya + yr.abs() + r.abs(), 4, dtype,
              trans=act in R.ACT_TRANS, extra=1.5 * 2 * R.U32 * uabs)
        assert untouched(ybuf, off, C)
    assert untouched(zbuf, off, C) and untouched(rbuf, off, C)


def du_ref(act, zc, dyc, sc, sh):
    """-> du, the bound on its fp32 evaluation (see the module docstring)"""
    u, uabs = zc.double() * sc + sh, (zc.double() * sc).abs() + sh.abs()
    d, ad = R.act_grad(act, u)
    du = dyc.double() * d
    tol = R.TRANS * (1 + d.abs()) if act in R.ACT_TRANS else 0.0
    return du, dyc.double().abs() * (2 * R.U32 * uabs + 4 * R.U32 * ad + tol) + R.U32 * du.abs()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,Ct,off', LAYOUTS)
@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_SILU, R.ACT_LEAKY])
def test_bn_bwd_reduce_and_apply(act, M, C, Ct, off, dtype):
    call, ptr, stream = _lib()
    gen = gen_for(M, C, Ct, off, act, 1)
    zc, dyc = randn((M, C), gen, dtype, 1.5), randn((M, C), gen, dtype)
    (sc, sh, inv, mu, ca, cb, cc), (scale, shift, invstd, mean, cad, cbd, ccd) = coefs(C, gen, 'pspspss')
    zbuf, z = slab(zc, Ct, off)
    gbuf, dy = slab(dyc, Ct, off)
    du, edu = du_ref(act, zc, dyc, sc, sh)
    xhat = (zc.double() - mu) * inv

    P = partial_rows(call, ptr, dtype, z, Ct, dy, Ct, M, C)
    pdb, pdg = torch.full((P, C), float('nan'), device='cuda'), torch.full((P, C), float('nan'), device='cuda')
    call('dmy_bn_bwd_reduce', dcode(dtype), ptr(z), Ct, ptr(dy), Ct, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), act,
         M, C, ptr(pdb), ptr(pdg), stream())
    t2 = du * xhat
    check(f'bn_bwd_reduce_db_act{act}', pdb.double().sum(0), du.sum(0), du.abs().sum(0), M, F32, extra=edu.sum(0))
    check(f'bn_bwd_reduce_dg_act{act}', pdg.double().sum(0), t2.sum(0), t2.abs().sum(0), M, F32,
          extra=(edu * xhat.abs() + 3 * R.U32 * t2.abs()).sum(0))

    dbuf, dz = slab(torch.zeros(M, C, dtype=dtype), Ct, off)
    call('dmy_bn_bwd_apply', dcode(dtype), ptr(z), Ct, ptr(dy), Ct, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), act,
         ptr(cad), ptr(cbd), ptr(ccd), ptr(dz), Ct, M, C, stream())
    k2 = cc * inv
    check(f'bn_bwd_apply_act{act}', dz, ca * du + cb + cc * xhat,
          (ca * du).abs() + cb.abs() + k2.abs() * (zc.double().abs() + mu.abs()), 6, dtype, extra=ca.abs() * edu)
    assert untouched(dbuf, off, C) and untouched(zbuf, off, C) and untouched(gbuf, off, C)
