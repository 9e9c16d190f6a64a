"""The yardstick of the SyncBatchNorm tests: float64 numpy restatements of the slab exchange (csrc/bn.hip,
dmy_bn_sync_*) and of plain batch statistics.  A slot is (sum a[C], sum b[C], n): (sum x, sum x^2, pixels) in the
forward, (sum dy, sum dy * xhat, pixels) in the backward; a slab is one slot per rank."""
import numpy as np


def split_rows(M, sizes):
    """row ranges [(lo, hi)] of consecutive parts of the given sizes, which must cover M rows"""
    assert sum(sizes) == M and all(s > 0 for s in sizes), (M, sizes)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(edges[i]), int(edges[i + 1])) for i in range(len(sizes))]


def slot(a, b):
    """(sum a, sum b, n) of one rank's rows a, b: (n, C)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.sum(0), b.sum(0), float(a.shape[0])


def merge(slots):
    """the slots added in rank order -> (sum a, sum b, n)"""
    sa, sb, n = (np.array(v, np.float64, copy=True) for v in slots[0])
    for s in slots[1:]:
        sa, sb, n = sa + s[0], sb + s[1], n + s[2]
    return sa, sb, float(n)


def stats_from_sums(sa, sb, n, gamma, beta, eps):
    """bn_finalize_kernel's formulas in float64 -> dict(mean, var, unbiased, invstd, scale, shift)"""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = sa / n
    var = np.maximum(sb / n - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    return dict(mean=mean, var=var, unbiased=var * n / (n - 1) if n > 1 else var, invstd=invstd, scale=gamma * invstd,
                shift=beta - mean * gamma * invstd)


def batch_stats(x, gamma, beta, eps):
    """plain BatchNorm statistics of x: (M, C), two-pass in float64 (no E[x^2] - E[x]^2 cancellation)"""
    x = np.asarray(x, np.float64)
    n = float(x.shape[0])
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    invstd = 1.0 / np.sqrt(var + eps)
    return dict(mean=mean, var=var, unbiased=var * n / (n - 1) if n > 1 else var, invstd=invstd, scale=gamma * invstd,
                shift=beta - mean * gamma * invstd)


def running(rmean, rvar, st, momentum):
    """torch's running-statistics update with the unbiased variance"""
    return ((1 - momentum) * np.asarray(rmean, np.float64) + momentum * st['mean'],
            (1 - momentum) * np.asarray(rvar, np.float64) + momentum * st['unbiased'])


def bwd_from_slots(slots, rank, gamma, invstd):
    """SyncBatchNorm's backward rule: dbeta / dgamma are slot `rank`'s own sums, the apply coefficients (dz = ca * du +
    cb + cc * xhat) come from every slot over the global count -> dict(dbeta, dgamma, ca, cb, cc)"""
    sa, sb, n = merge(slots)
    k = np.asarray(gamma, np.float64) * np.asarray(invstd, np.float64)
    return dict(dbeta=np.asarray(slots[rank][0], np.float64), dgamma=np.asarray(slots[rank][1], np.float64), ca=k,
                cb=-k * sa / n, cc=-k * sb / n)


def rel_l2(got, want, floor=0.0):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want)) / max(float(np.linalg.norm(want)), floor, 1e-300)
