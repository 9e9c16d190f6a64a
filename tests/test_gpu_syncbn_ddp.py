"""GPU, world size 2 (two gloo ranks sharing cuda:0, as tests/test_gpu_ddp.py): SyncBatchNorm on the HIP path
(train.py:272-275, --sync-bn) against ONE process running plain BatchNorm2d on the concatenated batch through the same
kernels.

Loss: the fixed linear functional sum(y * r), r seeded per sample, so the ranks' losses add up to the loss of the
concatenated batch (ComputeLoss's per-batch means do not).

Layer level (one spawn runs every case): rank 0 holds sample 0, rank 1 samples 1-3, 8 x 8 maps, one case per BN funnel
-- Conv(8, 16, 3); the bf16 1x1 Conv(64, 64) of the fused 1x1 backward; SCConv (deferred affine / BnLink); DMConv (spd);
one ConvMix stage (act before BN).  Per rank: y and dx against its slice of the reference; the running statistics equal
on both ranks bit for bit and to the reference's; the ranks' dgamma / dbeta / dw summed against the reference's.
Bound: regrouping the partial rows is the only legitimate difference, so it is measured on the reference alone -- the
batch against the same batch in reversed sample order, largest relative L2 per tensor class and storage type over the
cases -- and the bound is four times that (a factor two each for the second split point and for bf16 storage rounding of
z).  Measured spreads: DESIGN.md §5 (SyncBatchNorm).
Negative control: the Conv(8, 16, 3) case with the BN left unconverted misses that bound on running_mean.

Model level: the width-0.125 DMA topology of tests/golden/model_dma.npz @128, 2 images per rank, fp32, deterministic
mode, under torch DDP and under ArenaDDP: every parameter gradient after the all-reduce, times the world size, against
the single-process gradient of the 4-image batch, relative L2 <= 2e-3 per tensor with tests/test_gpu_ddp.py's floor (1e-3
of the largest gradient norm); the running statistics equal on both ranks bit for bit and within the same bound of the
reference's, with the same floor among themselves (1e-3 of the largest running-statistic norm): model.8.cv1 / cv2 see
an input whose channel means cancel, so their running_mean is rounding noise, norm 3.9e-9 in the reference itself
against 1e-2 .. 3e-1 for the other layers, and no relative figure means anything there (measured without the floor:
0.87 on those two tensors, 8.6e-7 on the worst of the other 128).

Fallbacks: a converted model in eval(), and one with no process group, equal the unconverted model bit for bit; a
converted layer under torch.cuda.graph capture at world size 2 raises before any launch.

Process rules: two ranks plus the parent, init_process_group(timeout=60 s) so a dead rank turns its peer's wait into an
error, mp.spawn(join=True), the group destroyed in a finally, tensors handed over through a temporary directory."""
import os
import tempfile
from datetime import timedelta

import pytest
import torch

from test_gpu_ddp import _free_port, _model, _setup

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32, BF16 = torch.float32, torch.bfloat16
WORLD = 2
SPLIT = [[0], [1, 2, 3]]  # the samples of rank 0 and rank 1 at layer level
HW = 8
CLASSES = ('y', 'dx', 'running', 'dbn', 'dw')


def _layer(name):
    """-> (module with seeded parameters and BN statistics, input channels)"""
    _setup()
    from dmayolo.models import common as P
    torch.manual_seed(7)
    mod, c1 = {'conv3': lambda: (P.Conv(8, 16, 3), 8),
               'conv1x1': lambda: (P.Conv(64, 64, 1), 64),
               'scconv': lambda: (P.SCConv(16, 16, 1), 16),
               'dmconv': lambda: (P.DMConv(8, 16), 8),
               'convmix': lambda: (P.ConvMix(16, 16).Conv_1x1, 16)}[name]()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return mod, c1


LAYER_CASES = [('conv3', F32), ('conv3', BF16), ('conv1x1', BF16), ('scconv', F32), ('scconv', BF16), ('dmconv', F32),
               ('dmconv', BF16), ('convmix', F32), ('convmix', BF16)]
IDS = [f'{n}-{str(d)[6:]}' for n, d in LAYER_CASES]


def _sample(i, shape, salt):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 * salt + i))


def _run_layer(mod, c1, dtype, samples):
    """one forward + backward of sum(y * r) over the given samples -> dict of cpu tensors, keyed by tensor class"""
    mod = mod.cuda().train()
    x = torch.stack([_sample(i, (c1, HW, HW), 1) for i in samples]).to(dtype).cuda().contiguous(memory_format=CL)
    x.requires_grad_(True)
    y = mod(x)
    r = torch.stack([_sample(i, tuple(y.shape[1:]), 2) for i in samples]).cuda()
    (y.float() * r).sum().backward()
    torch.cuda.synchronize()
    out = {'y': y.detach().float().cpu(), 'dx': x.grad.float().cpu()}
    for k, p in mod.named_parameters():
        bn = k.rsplit('.', 1)[0]
        is_bn = isinstance(mod.get_submodule(bn) if bn != k else mod, torch.nn.modules.batchnorm._BatchNorm)
        out[('dbn.' if is_bn else 'dw.') + k] = p.grad.detach().float().cpu().clone()
    for k, b in mod.named_buffers():
        out[('nbt.' if k.endswith('num_batches_tracked') else 'running.') + k] = b.detach().cpu().clone()
    return out


def _init(rank, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=WORLD, timeout=timedelta(seconds=60))
    return dist


def _layer_worker(rank, port, td):
    _setup()
    import dmayolo.functional as Fn
    from dmayolo import _lib
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    dist = _init(rank, port)
    Fn.set_deterministic(True)
    try:
        res = {}
        for (name, dtype), cid in zip(LAYER_CASES, IDS):
            mod, c1 = _layer(name)
            names = []
            _lib.TRACE[0] = lambda n, a: names.append(n)
            try:
                res[cid] = _run_layer(convert_sync_batchnorm(mod), c1, dtype, SPLIT[rank])
            finally:
                _lib.TRACE[0] = None
            res[cid]['launches'] = names
        mod, c1 = _layer('conv3')  # negative control: the BN left unconverted sees its own rank's pixels only
        res['control'] = _run_layer(mod, c1, F32, SPLIT[rank])
        # graph capture: the converted layer raises before it launches anything; the empty capture is never replayed
        mod, c1 = _layer('conv3')
        mod = convert_sync_batchnorm(mod).cuda().train()
        x = torch.zeros(1, c1, HW, HW, device='cuda').contiguous(memory_format=CL).requires_grad_(True)
        names, msg = [], None
        graph = torch.cuda.CUDAGraph()
        _lib.TRACE[0] = lambda n, a: names.append(n)
        try:
            with torch.cuda.graph(graph):
                mod(x)
        except RuntimeError as e:
            msg = str(e)
        finally:
            _lib.TRACE[0] = None
        del graph
        res['capture'] = {'message': msg, 'launches': names}
        torch.cuda.synchronize()
        torch.save(res, os.path.join(td, f'layer{rank}.pt'))
        dist.barrier()
    finally:
        Fn.set_deterministic(False)
        dist.destroy_process_group()


def _rel(a, b, floor=0.0):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), floor, 1e-300)


def _cls(key):
    return key.split('.', 1)[0]


@pytest.fixture(scope='module')
def layer_runs():
    """-> (per-rank results of the one layer-level spawn, the single-process references, the measured spread per
    (storage type, tensor class))"""
    import torch.multiprocessing as mp
    import dmayolo.functional as Fn
    _setup()
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_layer_worker, args=(_free_port(), td), nprocs=WORLD, join=True)
        ranks = [torch.load(os.path.join(td, f'layer{r}.pt'), weights_only=False) for r in range(WORLD)]
    refs, spread = {}, {}
    Fn.set_deterministic(True)
    try:
        for (name, dtype), cid in zip(LAYER_CASES, IDS):
            fwd = _run_layer(*_layer(name), dtype, [0, 1, 2, 3])
            rev = _run_layer(*_layer(name), dtype, [3, 2, 1, 0])
            refs[cid] = fwd
            for k in fwd:
                if _cls(k) not in CLASSES:
                    continue
                other = rev[k].flip(0) if k in ('y', 'dx') else rev[k]
                key = (dtype, _cls(k))
                spread[key] = max(spread.get(key, 0.0), _rel(other, fwd[k]))
    finally:
        Fn.set_deterministic(False)
    for (dtype, c), v in sorted(spread.items(), key=str):
        print(f'reference spread under reversed sample order, {str(dtype)[6:]} {c}: {v:.3e}  (bound {4 * v:.3e})')
    return ranks, refs, spread


@pytest.mark.parametrize('name,dtype', LAYER_CASES, ids=IDS)
def test_layer_matches_single_process_batchnorm(layer_runs, name, dtype):
    ranks, refs, spread = layer_runs
    cid = IDS[LAYER_CASES.index((name, dtype))]
    ref, got = refs[cid], [r[cid] for r in ranks]
    bound = {c: 4 * spread[(dtype, c)] for c in CLASSES}
    for r in range(WORLD):
        assert 'dmy_bn_sync_pack' in got[r]['launches'] and 'dmy_bn_finalize' not in got[r]['launches']
        assert 'dmy_bn_sync_bwd_finalize' in got[r]['launches'] and 'dmy_bn_bwd_finalize' not in got[r]['launches']
        if name == 'conv1x1':  # the funnel this case is here for: dmy_conv1x1_bwd_bn_ok accepted the layer
            assert 'dmy_conv1x1_bwd_bn' in got[r]['launches']
        if name == 'dmconv':
            assert 'dmy_bn_bwd_reduce_s2d' in got[r]['launches']
        if name == 'scconv' and dtype == BF16:
            assert 'dmy_scgate_bn_bwd' in got[r]['launches']
        if name == 'convmix':
            assert 'dmy_actbn_stats' in got[r]['launches']
    lo = 0
    worst = {}
    for r in range(WORLD):  # each rank's y and dx against its slice
        n = len(SPLIT[r])
        for k in ('y', 'dx'):
            e = _rel(got[r][k], ref[k][lo:lo + n])
            print(f'{cid} rank {r} {k}: {e:.3e} (bound {bound[k]:.3e})')
            worst[k] = max(worst.get(k, 0.0), e)
        lo += n
    for k in ref:
        c = _cls(k)
        if c == 'nbt':
            assert torch.equal(got[0][k], ref[k]) and torch.equal(got[1][k], ref[k]), k
        elif c == 'running':
            assert torch.equal(got[0][k], got[1][k]), f'{k}: the ranks hold different running statistics'
            e = _rel(got[0][k], ref[k])
            print(f'{cid} {k}: {e:.3e} (bound {bound[c]:.3e})')
            worst[c] = max(worst.get(c, 0.0), e)
        elif c in ('dbn', 'dw'):
            e = _rel(got[0][k] + got[1][k], ref[k])
            print(f'{cid} sum over ranks {k}: {e:.3e} (bound {bound[c]:.3e})')
            worst[c] = max(worst.get(c, 0.0), e)
    for c, e in worst.items():
        assert e <= bound[c], (cid, c, e, bound[c])


def test_unconverted_bn_misses_the_bound(layer_runs):
    """the negative control: plain BatchNorm2d under the same split sees one rank's pixels, so its running_mean is
    off the whole-batch reference by far more than any regrouping"""
    ranks, refs, spread = layer_runs
    ref = refs['conv3-float32']
    bound = 4 * spread[(F32, 'running')]
    errs = [_rel(r['control']['running.bn.running_mean'], ref['running.bn.running_mean']) for r in ranks]
    print(f'unconverted running_mean error per rank: {errs} (bound {bound:.3e})')
    assert all(e > bound for e in errs), (errs, bound)
    assert not torch.equal(ranks[0]['control']['running.bn.running_mean'], ranks[1]['control']['running.bn.running_mean'])


def test_graph_capture_raises_before_any_launch(layer_runs):
    ranks, _, _ = layer_runs
    for r in ranks:
        msg = r['capture']['message']
        assert msg is not None and 'SyncBatchNorm' in msg and 'graph capture' in msg, msg
        assert r['capture']['launches'] == [], r['capture']['launches']


# ------------------------------------------------------------------ model level

BS, IMG = 2, 128


def _images(rank):
    from dmayolo.synthetic import images
    return images(BS, IMG, seed=1 + rank, device='cuda')


def _model_loss(out, first):
    """sum(y * r) over every head map, r seeded per sample (global sample index first + i) and level"""
    outs = [out] if torch.is_tensor(out) else list(out)
    loss = 0.0
    for lv, o in enumerate(outs):
        r = torch.stack([_sample(first + i, tuple(o.shape[1:]), 3 + lv) for i in range(o.shape[0])]).cuda()
        loss = loss + (o.float() * r).sum()
    return loss


def _state(model):
    return {k: b.detach().cpu().clone() for k, b in model.named_buffers()}


def _model_worker(rank, port, td, reducer):
    _setup()
    import dmayolo.functional as Fn
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    dist = _init(rank, port)
    Fn.set_deterministic(True)
    net = None
    try:
        model, _, _ = _model('dma')
        model = convert_sync_batchnorm(model)
        if reducer == 'torch':
            net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[0], output_device=0)
        else:
            from dmayolo.ddp import ArenaDDP
            net = ArenaDDP(model, bucket_cap_mb=1.0, first_bucket_mb=0.25)
        _model_loss(net(_images(rank)), BS * rank).backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
        torch.save({'grads': grads, 'state': _state(model)}, os.path.join(td, f'model{rank}.pt'))
        dist.barrier()
    finally:
        if reducer != 'torch' and net is not None:
            net.close()
        Fn.set_deterministic(False)
        dist.destroy_process_group()


@pytest.fixture(scope='module')
def model_ref():
    """the single-process gradient of the 4-image batch through plain BatchNorm2d"""
    import dmayolo.functional as Fn
    _setup()
    Fn.set_deterministic(True)
    try:
        model, _, _ = _model('dma')
        _model_loss(model(torch.cat([_images(0), _images(1)])), 0).backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
        return grads, _state(model)
    finally:
        Fn.set_deterministic(False)


@pytest.mark.parametrize('reducer', ['torch', 'arena'])
def test_model_gradients_match_single_process(model_ref, reducer):
    import torch.multiprocessing as mp
    exp, state = model_ref
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_model_worker, args=(_free_port(), td, reducer), nprocs=WORLD, join=True)
        got = [torch.load(os.path.join(td, f'model{r}.pt'), weights_only=False) for r in range(WORLD)]
    assert set(got[0]['grads']) == set(exp) and len(exp) > 100
    gmax = max(float(v.norm()) for v in exp.values())
    worst = (-1.0, '')
    for k, v in exp.items():
        assert torch.equal(got[0]['grads'][k], got[1]['grads'][k]), f'{k}: the ranks hold different reduced gradients'
        worst = max(worst, (_rel(got[0]['grads'][k] * WORLD, v, 1e-3 * gmax), k))
    print(f'dma {reducer}: {len(exp)} gradients, worst relative L2 {worst[0]:.2e} ({worst[1]})')
    assert worst[0] <= 2e-3, worst
    errs = []
    smax = max(float(v.norm()) for k, v in state.items() if k.endswith(('running_mean', 'running_var')))
    for k, v in state.items():
        assert torch.equal(got[0]['state'][k], got[1]['state'][k]), f'{k}: the ranks hold different buffers'
        if k.endswith('num_batches_tracked'):
            assert torch.equal(got[0]['state'][k], v), k
        elif k.endswith(('running_mean', 'running_var')):
            g = got[0]['state'][k]
            errs.append((_rel(g, v, 1e-3 * smax), k, float(v.norm()), float((g - v).norm())))
    for e, k, nv, nd in sorted(errs, reverse=True)[:4]:
        print(f'dma {reducer}: {k} relative L2 {e:.2e} (|ref| {nv:.3e}, |diff| {nd:.3e})')
    sworst, n = max(errs)[:2], len(errs)
    print(f'dma {reducer}: {n} running statistics, worst relative L2 {sworst[0]:.2e} ({sworst[1]})')
    assert n > 100 and sworst[0] <= 2e-3, sworst


# ------------------------------------------------------------------ fallbacks (one process, no process group)

@pytest.mark.parametrize('how', ['helper', 'torch'])
def test_converted_model_without_a_group_equals_the_unconverted_one(how):
    """train mode with torch.distributed not initialised, then eval mode: outputs, gradients and running statistics
    bit-identical to the unconverted model's (the converted layers take the local path); converting with torch's own
    converter before the first forward works as well"""
    import copy
    import torch.distributed as dist
    import dmayolo.functional as Fn
    from dmayolo.utils.torch_utils import convert_sync_batchnorm
    _setup()
    assert not dist.is_initialized()
    Fn.set_deterministic(True)
    try:
        base, _, _ = _model('yolov5n')
        conv = copy.deepcopy(base)
        conv = convert_sync_batchnorm(conv) if how == 'helper' else torch.nn.SyncBatchNorm.convert_sync_batchnorm(conv)
        assert any(isinstance(m, torch.nn.SyncBatchNorm) for m in conv.modules())
        x = _images(0)
        res = []
        for m in (base, conv):
            _model_loss(m(x), 0).backward()
            grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
            m.eval()
            with torch.no_grad():
                y = m(x)
            res.append((grads, _state(m), (y[0] if isinstance(y, (tuple, list)) else y).clone()))
        torch.cuda.synchronize()
    finally:
        Fn.set_deterministic(False)
    (ga, sa, ya), (gb, sb, yb) = res
    assert set(ga) == set(gb) and set(sa) == set(sb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(ya, yb)
