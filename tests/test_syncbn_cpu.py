"""CPU: the host side of SyncBatchNorm (--sync-bn, train.py:272-275).  The three slab entry points are declared and
bound; a converted model groups its parameters and keeps its state dict as the unconverted one; a converted model with
no process group takes no exchange; and the float64 restatement of the slot merge (tests/syncbn_ref.py) equals plain
batch statistics for random splits, parts of 1 and 2 rows included.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import syncbn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'dma-yolo_amd', 'dmayolo', 'configs', 'yolov5n.yaml')
NEW = ('dmy_bn_sync_pack', 'dmy_bn_sync_finalize', 'dmy_bn_sync_bwd_finalize')


def _model():
    from dmayolo.models.yolo import Model
    torch.manual_seed(0)
    return Model(CFG, nc=10, act_dtype=torch.float32)


def test_slab_entries_are_declared_and_bound():
    from dmayolo import _lib
    hdr = open(os.path.join(ROOT, 'include', 'dmayolo.h')).read()
    for name in NEW:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    # the slab is passed by pointer, the pixel count of the pack as a double
    assert _lib.SIGNATURES['dmy_bn_sync_pack'][4] is _lib.D
    # finalize: dmy_bn_finalize's arguments with (slab, R) for (psum, psq, P) and no host-side count
    assert _lib.SIGNATURES['dmy_bn_sync_finalize'][3:] == _lib.SIGNATURES['dmy_bn_finalize'][5:]
    assert _lib.SIGNATURES['dmy_bn_sync_bwd_finalize'][4:] == _lib.SIGNATURES['dmy_bn_bwd_finalize'][5:]


def test_bad_slab_arguments_are_refused_before_any_launch():
    """hipErrorInvalidValue (1) for a null slab, a rank outside [0, R) and an empty channel range: host checks only"""
    import ctypes
    from dmayolo import _lib
    p = ctypes.c_void_p(4096)
    assert _lib.lib.dmy_bn_sync_pack(p, p, 4, 8, 4.0, None, 2, 0, None) == 1
    assert _lib.lib.dmy_bn_sync_pack(p, p, 4, 8, 4.0, p, 2, 2, None) == 1
    assert _lib.lib.dmy_bn_sync_pack(p, p, 4, 8, 4.0, p, 2, -1, None) == 1
    assert _lib.lib.dmy_bn_sync_pack(p, p, 4, 0, 4.0, p, 2, 0, None) == 1
    assert _lib.lib.dmy_bn_sync_finalize(p, 0, 8, p, p, p, p, p, 0.03, 1e-3, 1, p, p, p, p, None) == 1
    assert _lib.lib.dmy_bn_sync_bwd_finalize(p, 2, 2, 8, p, p, p, p, p, p, p, None) == 1


def test_param_groups_of_a_converted_model():
    """BN weights stay in the no-decay group: the same parameters, group by group, as before the conversion"""
    from dmayolo.optim import param_groups
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    m = _model()
    before = [[id(p) for p in g] for g in param_groups(m)]
    nbn = sum(isinstance(v, nn.BatchNorm2d) for v in m.modules())
    assert nbn > 0 and len(before[0]) == nbn
    m = convert_sync_batchnorm(m)
    assert not any(isinstance(v, nn.BatchNorm2d) for v in m.modules())
    assert sum(isinstance(v, nn.SyncBatchNorm) for v in m.modules()) == nbn
    after = [[id(p) for p in g] for g in param_groups(m)]
    assert [len(g) for g in after] == [len(g) for g in before]
    assert after == before
    # torch's own converter on a model that has not run gives the same grouping
    m2 = nn.SyncBatchNorm.convert_sync_batchnorm(_model())
    assert [len(g) for g in param_groups(m2)] == [len(g) for g in before]


def test_convert_keeps_the_state_dict():
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    m = _model()
    with torch.no_grad():
        for v in m.modules():  # statistics and hyper-parameters that differ from a fresh module's
            if isinstance(v, nn.BatchNorm2d):
                v.running_mean.uniform_(-1, 1)
                v.running_var.uniform_(0.5, 2)
                v.num_batches_tracked.fill_(7)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    eps = {n: (v.eps, v.momentum) for n, v in m.named_modules() if isinstance(v, nn.BatchNorm2d)}
    c = convert_sync_batchnorm(m)
    sd2 = c.state_dict()
    assert list(sd2) == list(sd)
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k
    assert {n: (v.eps, v.momentum) for n, v in c.named_modules() if isinstance(v, nn.SyncBatchNorm)} == eps
    assert all(e == (1e-3, 0.03) for e in eps.values())
    # checkpoints load both ways
    _model().load_state_dict(sd2)
    c.load_state_dict(sd)


def test_convert_drops_specs_that_hold_a_replaced_bn():
    import dmayolo.functional as Fn
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    m = _model()
    convs = [(v.conv, v.bn) for v in m.modules() if hasattr(v, 'conv') and isinstance(getattr(v, 'bn', None), nn.BatchNorm2d)]
    assert convs
    specs = [Fn.spec_for(c, 1, 0, Fn.ACT_SILU, b) for c, b in convs]
    assert all(c in Fn._SPECS for c, _ in convs)
    gen = Fn.PARAM_GEN[0]
    convert_sync_batchnorm(m)
    assert not any(c in Fn._SPECS for c, _ in convs) and Fn.PARAM_GEN[0] > gen
    for (c, old), sp in zip(convs, specs):
        new = [v for v in m.modules() if getattr(v, 'conv', None) is c][0].bn
        assert isinstance(new, nn.SyncBatchNorm) and new is not old
        assert Fn.spec_for(c, 1, 0, Fn.ACT_SILU, new).bn is new and sp.bn is old


def test_no_process_group_means_no_exchange():
    """the predicate of torch.nn.SyncBatchNorm.forward: a converted layer synchronises only in train mode inside an
    initialised process group of more than one rank"""
    import torch.distributed as dist
    import dmayolo.functional as Fn
    assert not dist.is_initialized()
    sbn, bn = nn.SyncBatchNorm(8), nn.BatchNorm2d(8)
    assert Fn._bn_sync(sbn, True) is None and Fn._bn_sync(sbn, False) is None
    assert Fn._bn_sync(bn, True) is None and Fn._bn_sync(None, False) is None


@pytest.mark.parametrize('seed', range(6))
def test_slot_merge_equals_batch_statistics(seed):
    """random row splits into 1..4 parts (sizes 1 and 2 forced in): the merged slots' statistics, running update and
    backward coefficients equal those of the whole batch to float64 rounding of the E[x^2] - E[x]^2 form"""
    rng = np.random.default_rng(seed)
    C, R = int(rng.integers(1, 9)), 1 + seed % 4
    sizes = [int(s) for s in rng.integers(1, 40, R)]
    sizes[0] = 1 + seed % 2  # a part of one row (even seeds) or two rows (odd seeds)
    M = sum(sizes)
    if M == 1:
        sizes, M = [1, 1], 2
    x = rng.normal(0.3, 1.7, (M, C))
    gamma, beta, eps, mom = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.3, C), 1e-3, 0.03
    parts = ref.split_rows(M, sizes)
    slots = [ref.slot(x[lo:hi], x[lo:hi] ** 2) for lo, hi in parts]
    assert ref.merge(slots)[2] == M
    got = ref.stats_from_sums(*ref.merge(slots), gamma, beta, eps)
    want = ref.batch_stats(x, gamma, beta, eps)
    # E[x^2] - E[x]^2 loses |mean|^2 / var of the 2^-53 relative precision; here that ratio is below 1e3
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)
    rm, rv = rng.normal(0, 1, C), rng.uniform(0.5, 2, C)
    for g, w in zip(ref.running(rm, rv, got, mom), ref.running(rm, rv, want, mom)):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12)
    # backward: the ranks' dgamma / dbeta sum to the whole batch's, the coefficients are the whole batch's
    dy = rng.normal(0, 1, (M, C))
    xhat = (x - want['mean']) * want['invstd']
    bslots = [ref.slot(dy[lo:hi], (dy * xhat)[lo:hi]) for lo, hi in parts]
    whole = ref.bwd_from_slots([ref.slot(dy, dy * xhat)], 0, gamma, want['invstd'])
    per_rank = [ref.bwd_from_slots(bslots, r, gamma, want['invstd']) for r in range(len(parts))]
    for k in ('dbeta', 'dgamma'):
        np.testing.assert_allclose(sum(p[k] for p in per_rank), whole[k], rtol=1e-12, atol=1e-12)
    for p in per_rank:
        for k in ('ca', 'cb', 'cc'):
            np.testing.assert_allclose(p[k], whole[k], rtol=1e-12, atol=1e-12)
    # ... and they are the gradient of the whole-batch BatchNorm: dz = ca * dy + cb + cc * xhat
    k_ = gamma * want['invstd']
    dz = k_ * (dy - dy.mean(0) - xhat * (dy * xhat).mean(0))
    np.testing.assert_allclose(whole['ca'] * dy + whole['cb'] + whole['cc'] * xhat, dz, rtol=1e-11, atol=1e-12)
