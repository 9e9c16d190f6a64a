"""GPU: ComputeLoss with the focal wrapper (hyp['fl_gamma'] > 0) and autobalance on the HIP path.

Reference parity against the fixtures of tools/gen_golden.py gen_focal() (the reference's own ComputeLoss), the cases
those do not hold against the float64 restatement tests/focal_ref.py (pinned to the fixtures by test_focal_ref.py),
and the contracts around them: no host synchronisation in a step, an unchanged default path, run-to-run bit
equality, GraphedTrainStep.  Tolerances are test_gpu_loss_nms.py::test_loss_and_grad's: loss / items rtol 1e-5
atol 1e-6, gradients rtol 1e-4 atol 1e-6 * max(1, |g|max); balance rtol 1e-5."""
import copy
import os
import types

import pytest
import torch

from focal_ref import FocalComputeLoss
from golden_util import Fixture

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dma-yolo_amd', 'dmayolo', 'configs')


def _loss_obj(fx, autobalance=False, nc=None, **hyp):
    from dmayolo.utils.loss import ComputeLoss
    meta = fx.meta
    det = types.SimpleNamespace(nl=3, na=3, nc=nc or meta['nc'], anchors=fx.t('anchors').cuda(),
                                stride=torch.tensor(meta['stride'], dtype=torch.float32))
    model = types.SimpleNamespace(hyp=dict(meta['hyp'], **hyp), model=[det])
    return ComputeLoss(model, autobalance=autobalance)


def _ref_obj(fx, autobalance=False, nc=None, **hyp):
    m = fx.meta
    return FocalComputeLoss(fx.t('anchors'), dict(m['hyp'], **hyp), nc or m['nc'], m['stride'], autobalance=autobalance)


def _close_lig(loss, items, grads, rloss, ritems, rgrads, grad_rtol=1e-4):
    torch.testing.assert_close(loss.float().cpu(), rloss.float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(items.float().cpu(), ritems.float(), rtol=1e-5, atol=1e-6)
    for g, r in zip(grads, rgrads):
        r = r.float()
        assert bool(torch.isfinite(g).all())
        torch.testing.assert_close(g.float().cpu(), r, rtol=grad_rtol, atol=1e-6 * max(1.0, float(r.abs().max())))


def _run(cl, ps, targets):
    ps = [p.detach().clone().requires_grad_(True) for p in ps]
    loss, items = cl(ps, targets)
    loss.backward()
    return loss.detach(), items, [p.grad for p in ps]


def _run_ref(ref, ps, targets):
    """the float64 helper on the CPU, fed exactly the values the kernels read (a bf16 p through .float())"""
    pp = [p.detach().float().cpu().double().requires_grad_(True) for p in ps]
    loss, items = ref(pp, targets.cpu())
    loss.backward()
    return loss.detach(), items, [p.grad for p in pp]


# ---------------------------------------------------------------- 1. reference parity
@pytest.mark.parametrize('name', ['focal_visdrone', 'focal_scratch_ls', 'focal_g05'])
@pytest.mark.parametrize('layout', ['contiguous', 'nhwc'])
def test_focal_loss_and_grad_vs_reference(name, layout):
    fx = Fixture(name)
    cl = _loss_obj(fx)
    ps = []
    for i in range(3):
        p = fx.t(f'p.{i}').cuda()
        if layout == 'nhwc':  # the Detect head's native layout: [N,H,W,na,no] permuted view
            p = p.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
        ps.append(p.requires_grad_(True))
    loss, items = cl(ps, fx.t('targets').cuda())
    loss.backward()
    print(name, layout, 'loss', float(loss.detach()), float(fx.t('loss')), 'items', items.tolist(),
          fx.t('items').tolist())
    _close_lig(loss.detach(), items, [p.grad for p in ps], fx.t('loss'), fx.t('items'),
               [fx.t(f'gp.{i}') for i in range(3)])


# ---------------------------------------------------------------- 2. autobalance trajectory, no host sync
def _four_calls(fx, cl):
    """the fixture's four successive calls, eagerly: per call (loss, items, balance tensor copy), last call's grads"""
    t = fx.t('targets').cuda()
    out = []
    for k in range(fx.meta['calls']):
        ps = [fx.t(f'p.{i}')[k].cuda().requires_grad_(True) for i in range(3)]
        loss, items = cl(ps, t)
        out.append((loss.detach(), items, cl.balance_dev.clone()))
    loss.backward()
    return out, [p.grad for p in ps]


@pytest.mark.parametrize('name', ['focal_autobalance', 'focal_autobalance_g0'])
def test_autobalance_trajectory_vs_reference(name):
    fx = Fixture(name)
    ncall = fx.meta['calls']
    cl = _loss_obj(fx, autobalance=True)
    assert cl.ssi == fx.meta['ssi'] == 1
    assert cl.balance == [4.0, 1.0, 0.4]
    out, grads = _four_calls(fx, cl)
    for k, (loss, items, bal) in enumerate(out):
        print(name, k, float(loss), items.tolist(), bal.tolist(), fx.t('balance')[k].tolist())
        torch.testing.assert_close(loss.cpu(), fx.t('loss')[k], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(items.cpu(), fx.t('items')[k], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(bal.cpu(), fx.t('balance')[k], rtol=1e-5, atol=0)
    torch.testing.assert_close(torch.tensor(cl.balance, dtype=torch.float64), fx.t('balance')[-1], rtol=1e-5, atol=0)
    for i in range(3):
        g = fx.t(f'gp.{i}')
        torch.testing.assert_close(grads[i].cpu(), g, rtol=1e-4, atol=1e-6 * max(1.0, float(g.abs().max())))

    # the same four calls recorded into one graph by a fresh object: capture raises on any host synchronisation, and
    # one replay from the initial balance gives the eager results bit for bit (same kernels, same order)
    cl2 = _loss_obj(fx, autobalance=True)
    t = fx.t('targets').cuda()
    sp = [[fx.t(f'p.{i}')[k].cuda().requires_grad_(True) for i in range(3)] for k in range(ncall)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rec = []
    with torch.cuda.graph(graph):
        for k in range(ncall):
            loss, items = cl2(sp[k], t)
            rec.append((loss.detach(), items, cl2.balance_dev.clone()))
        loss.backward()
    assert cl2.balance == [4.0, 1.0, 0.4]  # capture launched nothing
    graph.replay()
    torch.cuda.synchronize()
    for (l1, i1, b1), (l2, i2, b2) in zip(out, rec):
        assert torch.equal(l1, l2) and torch.equal(i1, i2) and torch.equal(b1, b2)
    for g1, p2 in zip(grads, sp[-1]):
        assert torch.equal(g1, p2.grad)
    assert cl2.balance == cl.balance


# ---------------------------------------------------------------- 3. cases the fixtures do not hold
def _case(case):
    """(p list on the GPU, targets on the GPU for the product, targets for the helper, nc)"""
    fx = Fixture('focal_g05')  # nc 10, img 128: levels 16^2 / 8^2 / 4^2, bs 2
    nc = 1 if case == 'nc1' else fx.meta['nc']
    ps = [fx.t(f'p.{i}')[..., :5 + nc].contiguous().cuda() for i in range(3)]
    t = fx.t('targets')
    if nc == 1:
        t = t.clone()
        t[:, 1] = 0
    tp = t
    if case == 'no_targets':
        tp = t = torch.zeros((0, 6))
    elif case == 'zero_padded':  # GraphedTrainStep's static target buffer: zero rows after the real ones
        tp = torch.cat([t, torch.zeros((9, 6))], 0)
    elif case == 'shared_cell':  # several targets in one (b, a, gj, gi) cell, different classes and sizes
        extra = torch.tensor([[0, 1, 0.52, 0.48, 0.10, 0.12], [0, 2, 0.52, 0.48, 0.12, 0.10],
                              [0, 3, 0.521, 0.481, 0.09, 0.14], [1, 4, 0.30, 0.70, 0.20, 0.25],
                              [1, 4, 0.30, 0.70, 0.25, 0.20]])
        tp = t = torch.cat([t, extra], 0)
    elif case == 'bf16':
        ps = [p.bfloat16() for p in ps]
    return fx, ps, tp.cuda(), t, nc


@pytest.mark.parametrize('case', ['nc1', 'no_targets', 'zero_padded', 'shared_cell', 'bf16'])
def test_focal_cases_vs_float64_helper(case):
    fx, ps, tp, t, nc = _case(case)
    cl = _loss_obj(fx, nc=nc, fl_gamma=1.5)
    loss, items, grads = _run(cl, ps, tp)
    rloss, ritems, rgrads = _run_ref(_ref_obj(fx, nc=nc, fl_gamma=1.5), ps, t)
    print(case, float(loss), float(rloss), items.tolist(), ritems.tolist())
    if case in ('nc1', 'no_targets'):
        assert float(items[2]) == 0.0
    if case == 'no_targets':
        assert float(items[0]) == 0.0
    if case == 'shared_cell':
        from oracle.loss import build_targets
        r = build_targets([p.shape for p in ps], t, fx.t('anchors'), fx.meta['hyp']['anchor_t'])[1]
        cells = torch.stack([r['b'], r['a'], r['gj'], r['gi']], 1)
        assert cells.unique(dim=0, return_counts=True)[1].max() >= 3
    # bf16 p: the gradient leaves the kernel rounded to bf16, one rounding of relative size 2^-8
    _close_lig(loss, items, grads, rloss, ritems, rgrads, grad_rtol=1e-4 + (2.0 ** -8 if case == 'bf16' else 0.0))
    assert all(g.dtype == p.dtype for g, p in zip(grads, ps))


@pytest.mark.parametrize('gamma', [1.0, 1.5, 2.0, 0.7, 0.5])
def test_every_gamma_path_vs_float64_helper(gamma):
    """gamma 1 / 1.5 / 2 take the multiply / sqrtf forms, any other gamma powf; label smoothing makes the class
    targets soft as well"""
    fx, ps, tp, t, nc = _case('plain')
    loss, items, grads = _run(_loss_obj(fx, fl_gamma=gamma, label_smoothing=0.1), ps, tp)
    rloss, ritems, rgrads = _run_ref(_ref_obj(fx, fl_gamma=gamma, label_smoothing=0.1), ps, t)
    _close_lig(loss, items, grads, rloss, ritems, rgrads)


# ---------------------------------------------------------------- 4. saturation
@pytest.mark.parametrize('gamma', [1.5, 0.5])
def test_saturated_logits_finite_and_match_helper(gamma):
    """objectness and class logits of +-30 and +-100 on target cells and on non-target cells: where the fp32 sigmoid
    has saturated onto the target 1 - p_t is exactly 0, the loss element is 0 and the second gradient term is taken
    as 0 (torch gives NaN there for gamma < 1); the true values are below the atol"""
    from oracle.loss import build_targets
    fx, ps, tp, t, nc = _case('plain')
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
    tg = build_targets([p.shape for p in ps], t, fx.t('anchors'), fx.meta['hyp']['anchor_t'])
    for i, p in enumerate(ps):
        r = tg[i]
        n = r['b'].numel()
        assert n > 0
        pc = p.cpu()
        # target cells: every objectness / class logit saturated, the sign pattern shifting with target and channel
        k = (torch.arange(n)[:, None] + torch.arange(nc + 1)[None]) % 4
        pc[r['b'], r['a'], r['gj'], r['gi'], 4:] = vals[k]
        # every third cell (targets or not): saturated objectness
        flat = pc.view(-1, nc + 5)
        idx = torch.arange(0, flat.shape[0], 3)
        keep = flat[idx, 4].abs() < 29  # not one of the target cells just written
        flat[idx[keep], 4] = vals[idx[keep] % 4]
        ps[i] = pc.cuda()
    loss, items, grads = _run(_loss_obj(fx, fl_gamma=gamma), ps, tp)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(items).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    rloss, ritems, rgrads = _run_ref(_ref_obj(fx, fl_gamma=gamma), ps, t)
    assert all(bool(torch.isfinite(g).all()) for g in rgrads)
    print(gamma, float(loss), float(rloss), items.tolist(), ritems.tolist())
    _close_lig(loss, items, grads, rloss, ritems, rgrads)


# ---------------------------------------------------------------- 5. unchanged default
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_default_path_is_the_original_entries(dtype):
    """fl_gamma == 0 and autobalance off: ComputeLoss equals the dmy_yolo_loss_level / dmy_yolo_loss_finalize /
    dmy_loss_grad entries called directly, bit for bit"""
    from dmayolo.functional import call, ptr, stream, dcode
    from dmayolo.utils.loss import _build_level
    fx = Fixture('loss_VisDrone')
    assert fx.meta['hyp']['fl_gamma'] == 0
    cl = _loss_obj(fx)
    assert cl.balance_dev is None
    ps = [fx.t(f'p.{i}').cuda().to(dtype) for i in range(3)]
    ps[1] = ps[1].permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    t = fx.t('targets').cuda()
    up = torch.tensor([3.0], device='cuda')
    run = [p.detach().requires_grad_(True) for p in ps]
    loss, items = cl(run, t)
    loss.backward(up)
    assert cl.balance_dev is None and cl.balance == [4.0, 1.0, 0.4]

    h, nc, bs = fx.meta['hyp'], fx.meta['nc'], ps[0].shape[0]
    PR = call('dmy_yolo_loss_part_rows')
    part = torch.zeros(3 * PR, dtype=torch.float32, device='cuda')
    balance = [4.0, 1.0, 0.4]
    dps = []
    keep = []
    for i, pi in enumerate(ps):
        N, na, H, W, no = pi.shape
        ii, tbox, anch, cnt, cap = _build_level(t, t.shape[0], cl.anchors[i], na, H, W, h['anchor_t'], pi.device)
        G = torch.zeros_like(pi, dtype=torch.float32)
        tobj = torch.zeros(N * na * H * W, dtype=torch.float32, device='cuda')
        tgrad = torch.empty((cap, 4 + nc), dtype=torch.float32, device='cuda')
        links = torch.empty(N * na * H * W + cap, dtype=torch.int32, device='cuda')
        s = pi.stride()
        call('dmy_yolo_loss_level', dcode(pi), ptr(pi), s[0], s[1], s[2], s[3], N, na, H, W, no, nc, float(h['box']),
             float(h['obj']), float(h['cls']), float(h['cls_pw']), float(h['obj_pw']), 1.0, 0.0, balance[i], float(bs),
             ptr(ii[0]), ptr(ii[1]), ptr(ii[2]), ptr(ii[3]), ptr(ii[4]), ptr(tbox), ptr(anch), ptr(cnt), cap, ptr(G),
             ptr(tobj), ptr(part[PR * i:]), ptr(tgrad), ptr(links), stream())
        dp = torch.empty_like(G, dtype=dtype)
        call('dmy_loss_grad', 1 if dtype == torch.bfloat16 else 0, ptr(G), ptr(up), ptr(dp), G.numel(), stream())
        dps.append(dp)
        keep.append((ii, tbox, anch, tobj, tgrad, links, G))
    l2 = torch.empty(1, device='cuda')
    i2 = torch.empty(3, device='cuda')
    call('dmy_yolo_loss_finalize', ptr(part), 3, float(h['box']), float(h['obj']), float(h['cls']), float(bs), ptr(l2),
         ptr(i2), stream())
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), l2) and torch.equal(items, i2)
    for p, dp in zip(run, dps):
        assert torch.equal(p.grad, dp)


# ---------------------------------------------------------------- 6. determinism
def test_autobalance_focal_bitwise_repeatable():
    fx = Fixture('focal_autobalance')
    a, ga = _four_calls(fx, _loss_obj(fx, autobalance=True))
    b, gb = _four_calls(fx, _loss_obj(fx, autobalance=True))
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert all(torch.equal(u, v) for u, v in zip(ga, gb))


# ---------------------------------------------------------------- 7. graphed step
def test_graphed_train_step_focal_autobalance_matches_eager():
    """yolov5n @64 bs 2, fl_gamma 1.5, autobalance: three GraphedTrainStep calls (one capturing call + two replays)
    against three eager steps of an identical copy.  As in test_gpu_model.py::test_graphed_train_step_matches_eager
    (deterministic mode: the same kernels on the same data) the bound is bit equality, here also for the balance,
    whose update kernel the graph replays."""
    import dmayolo.functional as Fn
    from dmayolo.models.yolo import Model
    from dmayolo.optim import FusedSGD
    from dmayolo.utils.loss import ComputeLoss
    from dmayolo.synthetic import targets as synth_targets, HYP_VISDRONE, scaled_hyp
    from dmayolo.train_graph import GraphedTrainStep
    Fn.set_deterministic(True)
    try:
        torch.manual_seed(0)
        m1 = Model(os.path.join(CFG, 'yolov5n.yaml'), nc=10, act_dtype=torch.float32).cuda().train()
        m1.hyp = dict(scaled_hyp(HYP_VISDRONE, 10, 64, 3), fl_gamma=1.5)
        m2 = copy.deepcopy(m1)
        o1 = FusedSGD(m1.parameters(), lr=0.01, momentum=0.9, nesterov=True)
        o2 = FusedSGD(m2.parameters(), lr=0.01, momentum=0.9, nesterov=True)
        l1, l2 = ComputeLoss(m1, autobalance=True), ComputeLoss(m2, autobalance=True)
        assert l1.ssi == 1
        gstep = GraphedTrainStep(m2, l2, o2, tcap=16)
        g = torch.Generator().manual_seed(5)
        for i, nt_per in enumerate([3, 5, 4]):
            x = torch.randint(0, 256, (2, 3, 64, 64), generator=g, dtype=torch.uint8).cuda()
            t = synth_targets(2, 10, per_image=nt_per, seed=10 + i, device='cuda')
            o1.zero_grad(set_to_none=True)
            a, ai = l1(m1(x), t)
            a.backward()
            o1.step()
            b, bi = gstep(x, t)
            assert torch.equal(b, a.detach()) and torch.equal(bi, ai), (i, b, a)
        assert gstep.captures == 1
        assert l1.balance == l2.balance and l1.balance != [4.0, 1.0, 0.4] and l1.balance[1] == 1.0
    finally:
        Fn.set_deterministic(False)


def test_trainer_passes_autobalance_through():
    from dmayolo.models.yolo import Model
    from dmayolo.synthetic import HYP_VISDRONE, scaled_hyp
    from dmayolo.trainer import Trainer
    m = Model(os.path.join(CFG, 'yolov5n.yaml'), nc=10, act_dtype=torch.float32).cuda().train()
    m.hyp = dict(scaled_hyp(HYP_VISDRONE, 10, 64, 3), fl_gamma=1.5)
    tr = Trainer(m, m.hyp, batch_size=2, epochs=2, nb=2, ema=False, amp=False, autobalance=True)
    assert tr.compute_loss.autobalance and tr.compute_loss.ssi == 1 and tr.compute_loss.fl_gamma == 1.5
    assert not Trainer(copy.deepcopy(m), dict(m.hyp), batch_size=2, epochs=2, nb=2, ema=False,
                       amp=False).compute_loss.autobalance
