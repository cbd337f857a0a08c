"""GPU: gradient accumulation -- rt_grad_accum against float64 torch, and accumulation windows through the eager loop body, the
epoch loop and the replayed step against plain backward passes / plain steps of the existing code.

Kernel data: the three gradients of an element share their sign (magnitudes spread over 16 binades).  The accumulator must hold
torch's fp32 `g0 + g1` bit for bit, i.e. it carries one rounding of its own, up to 2^-24 |acc|; only where |acc| <= |g0 + g1 + g2|
(same signs) is that guaranteed to stay inside the 1-ulp gate on the average -- with cancellation the accumulator's rounding alone
can be any number of ulps of the result, whatever the kernel does.  FINISH itself adds and scales in double and rounds once.

Model gates are those of the project's eager-vs-graph comparisons (tests/test_backbone_variants_gpu.py): gradients rel-L2 1e-6,
norms 1e-4, weights 1e-7 -- the 4 % of the gradient buffer that backward accumulates with atomics keeps them from being bit gates.
"""
import ctypes
import socket

import pytest
import torch

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state

pytestmark = pytest.mark.gpu

LAYERS = (1, 1, 1, 1)


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------ the kernel
def _grads(n, seed):
    gen = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return [(sign * (1.0 + torch.rand(n, generator=gen)) * torch.exp2(torch.randint(-8, 9, (n,), generator=gen).float())).float().cuda()
            for _ in range(3)]


def _view(n, off, fill):
    """An n-element view `off` elements into a larger buffer filled with a sentinel (what lies around the view must stay)."""
    buf = torch.full((n + 9,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[off:off + n]


def _ulp_distance(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item()


def _check_finish(H, g, acc_before, g_before, s32, sq):
    # what FINISH is specified to compute, operation for operation: the fp32 accumulator and gradient added in double (exact: both
    # lie within 17 binades), scaled in double, rounded once to fp32 -- so the gate is bit equality; a kernel that added or scaled in
    # fp32 would be up to an ulp away
    ref = ((acc_before.double() + g_before.double()) * float(s32)).float()
    assert (ref != 0).all() and torch.equal(g, ref), _ulp_distance(g, ref)
    want = float((g.double() ** 2).sum())
    assert abs(float(sq) - want) <= 1e-4 * want, (float(sq), want)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1027, (1 << 20) + 7])
def test_kernel_vs_float64(hip, n, off):
    H = hip
    g0, g1, g2 = _grads(n, seed=n + off)
    gbuf, g = _view(n, off, 7.0)
    abuf, acc = _view(n, off, -3.0)
    ws = torch.empty(H.GRAD_ACCUM_SLOTS, dtype=torch.float32, device="cuda")
    sq = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)

    def untouched():
        for buf, fill in ((gbuf, 7.0), (abuf, -3.0)):
            assert (buf[:off] == fill).all() and (buf[off + n:] == fill).all()

    # first, add, finish(1/3)
    g.copy_(g0); H.grad_accum(H.ACCUM_FIRST, g, acc)
    assert torch.equal(acc, g0) and torch.equal(g, g0)
    g.copy_(g1); H.grad_accum(H.ACCUM_ADD, g, acc)
    assert torch.equal(acc, g0 + g1) and torch.equal(g, g1)            # one rounded add, bit for bit
    acc2 = acc.clone()
    g.copy_(g2); H.grad_accum(H.ACCUM_FINISH, g, acc, scale=float(third), partials=ws, out_sq=sq)
    assert torch.equal(acc, acc2)                                        # FINISH only reads the accumulator
    # against the float64 sum of the THREE gradients (the accumulator's own rounding included in the gate)
    ref3 = ((g0.double() + g1.double() + g2.double()) * float(third)).float()
    assert _ulp_distance(g, ref3) <= 1, _ulp_distance(g, ref3)
    _check_finish(H, g, acc2, g2, third, sq)
    untouched()
    by_value, sq_value = g.clone(), sq.clone()
    # the scale from a device word (the by-value argument is then ignored): the same bits; and the same bits from run to run
    s_dev = third.reshape(1).cuda()
    for _ in range(2):
        sq.fill_(-1.0)
        g.copy_(g2); H.grad_accum(H.ACCUM_FINISH, g, acc, scale=0.0, scale_dev=s_dev, partials=ws, out_sq=sq)
        assert torch.equal(g, by_value) and torch.equal(sq, sq_value)
    # first, finish(1/2)
    g.copy_(g0); H.grad_accum(H.ACCUM_FIRST, g, acc)
    g.copy_(g1); H.grad_accum(H.ACCUM_FINISH, g, acc, scale=0.5, partials=ws, out_sq=sq)
    _check_finish(H, g, g0, g1, torch.tensor(0.5), sq)
    untouched()


def test_kernel_with_differently_aligned_buffers(hip):
    """g one element off a 16-byte boundary, the accumulator on it: no common vector alignment, every element goes one by one."""
    H = hip
    n = 1027
    g0, g1, _ = _grads(n, seed=5)
    gbuf, g = _view(n, 1, 7.0)
    abuf, acc = _view(n, 0, -3.0)
    ws = torch.empty(H.GRAD_ACCUM_SLOTS, dtype=torch.float32, device="cuda")
    sq = torch.zeros(1, dtype=torch.float32, device="cuda")
    g.copy_(g0); H.grad_accum(H.ACCUM_FIRST, g, acc)
    assert torch.equal(acc, g0)
    g.copy_(g1); H.grad_accum(H.ACCUM_FINISH, g, acc, scale=0.5, partials=ws, out_sq=sq)
    _check_finish(H, g, g0, g1, torch.tensor(0.5), sq)
    assert gbuf[0] == 7.0 and (gbuf[1 + n:] == 7.0).all() and (abuf[n:] == -3.0).all()


def test_kernel_refuses_bad_arguments(hip):
    H = hip
    L = H.lib()
    g = torch.ones(64, dtype=torch.float32, device="cuda")
    acc = torch.full((64,), 2.0, dtype=torch.float32, device="cuda")
    ws = torch.zeros(H.GRAD_ACCUM_SLOTS, dtype=torch.float32, device="cuda")
    sq = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    null = ctypes.c_void_p(0)
    call = lambda mode, a, b, n, w, o: L.rt_grad_accum(mode, a, b, n, 0.5, null, w, o, null)      # noqa: E731
    BADARG, UNSUPPORTED = -1, -2
    assert call(H.ACCUM_ADD, null, p(acc), 64, null, null) == BADARG
    assert call(H.ACCUM_ADD, p(g), null, 64, null, null) == BADARG
    assert call(H.ACCUM_ADD, p(g), p(acc), 0, null, null) == BADARG
    assert call(H.ACCUM_ADD, p(g), p(acc), -4, null, null) == BADARG
    assert call(H.ACCUM_FINISH, p(g), p(acc), 64, null, p(sq)) == BADARG           # FINISH needs its workspace and its output
    assert call(H.ACCUM_FINISH, p(g), p(acc), 64, p(ws), null) == BADARG
    assert call(7, p(g), p(acc), 64, p(ws), p(sq)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (g == 1).all() and (acc == 2).all() and float(sq) == -1.0                # nothing was launched


# ------------------------------------------------------------------------------------------------ the model
def to_cuda(samples, targets):
    from reftr_amd.util.misc import NestedTensor
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].cuda(), samples["img_mask"].cuda())
    return s, [{k: v.cuda() for k, v in t.items()} for t in targets]


def make_batches(n):
    """Batch 0 = make_inputs("e2e_single"); batch j: the images (with their sentences and targets) in another order on odd j, the
    pixels scaled and the boxes moved -- same shapes, other gradients."""
    base_s, base_t = make_inputs("e2e_single", B=2, H=128, W=160, L=12)
    out = []
    for j in range(n):
        order = [1, 0] if j % 2 else [0, 1]
        s = {k: v[order].clone() for k, v in base_s.items()}
        s["img"] = s["img"] * (1.0 - 0.06 * j)
        t = [{"boxes": (base_t[b]["boxes"] + torch.tensor([0.02, -0.015, 0.01, 0.012]) * j).clamp(0.05, 0.95),
              "labels": base_t[b]["labels"].clone()} for b in order]
        out.append((s, t))
    return out


@pytest.fixture(scope="module")
def world():
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), resnet_layers=LAYERS)
    return {"ocfg": ocfg, "P": formula_state(param_shapes(ocfg)), "cpu": make_batches(5), "cuda": [to_cuda(*b) for b in make_batches(5)]}


def build(world, train=False):
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.models.reftr_transformer import RefTR
    from reftr_amd.optim import FusedAdamW
    cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), resnet_layers=LAYERS)
    model = RefTR(cfg, device="cuda")
    model.load_state_dict(world["P"], strict=True)
    model.eval()                                         # dropout off
    crit = CriterionVGMultiPhrase(O.weight_dict(world["ocfg"]), ["boxes"])
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    return model, crit, opt


@pytest.fixture()
def launched_head(monkeypatch):
    monkeypatch.setenv("REFTR_HEAD_FUSE", "0")           # the eager loop's head kernel on both sides, as the eager / graph comparisons do


@pytest.fixture(scope="module")
def plain_grads(world):
    """flat_g after a plain forward + backward (existing code only) of batches 0, 1, 2 at the initial weights: computed once."""
    import os
    from reftr_amd.engine_vg import _total, _zero_grad
    old = os.environ.get("REFTR_HEAD_FUSE")
    os.environ["REFTR_HEAD_FUSE"] = "0"
    try:
        model, crit, opt = build(world)
        out = []
        for s, tg in world["cuda"][:3]:
            total = _total(crit, crit(model(s), tg))
            _zero_grad(opt)
            total.backward()
            torch.cuda.synchronize()
            out.append(model.store.flat_g.clone())
    finally:
        if old is None:
            del os.environ["REFTR_HEAD_FUSE"]
        else:
            os.environ["REFTR_HEAD_FUSE"] = old
    return out


def test_eager_window_is_the_mean_of_plain_backward_passes(hip, world, plain_grads, launched_head):
    from reftr_amd.engine_vg import train_step
    mean = (plain_grads[0] + plain_grads[1]) / 2
    ref_model, _, ref_opt = build(world)
    ref_model.store.flat_g.copy_(mean)
    ref_opt.clip_grad_norm_(0.1)
    ref_opt.step()
    model, crit, opt = build(world)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    p0 = model.store.flat_p.clone()
    (s0, t0), (s1, t1) = world["cuda"][:2]
    r0 = train_step(model, crit, s0, t0, opt, sched, max_norm=0.1, accum_steps=2)
    assert r0[3] is None and opt.step_count == 0 and sched.last_epoch == 0 and opt.accum_count == 1
    assert torch.equal(model.store.flat_p, p0)
    r1 = train_step(model, crit, s1, t1, opt, sched, max_norm=0.1, accum_steps=2)
    torch.cuda.synchronize()
    want = float(mean.double().norm())
    g_rel, p_rel, n_rel = rel(model.store.flat_g, mean), rel(model.store.flat_p, ref_model.store.flat_p), abs(float(r1[3]) - want) / want
    print(f"\n[accum eager k=2] flat_g rel {g_rel:.2e}  grad norm rel {n_rel:.2e}  flat_p rel {p_rel:.2e}")
    assert g_rel < 1e-6
    assert n_rel < 1e-4
    assert p_rel < 1e-7
    assert opt.step_count == 1 and int(opt.step_dev) == 1 and opt.accum_count == 0
    assert sched.last_epoch == 1 and opt.param_groups[0]["lr"] == pytest.approx(0.5e-4)
    assert r0[0] > 0 and r1[0] > 0 and r0[0] != r1[0]


class _SnapLR(torch.optim.lr_scheduler.StepLR):
    """StepLR that keeps (weights, moments, step) as they are when the loop steps it: once per update."""

    def __init__(self, opt, model):
        self.snaps, self._model, self._live = [], model, False
        super().__init__(opt, step_size=100)
        self._live = True

    def step(self, *a):
        super().step(*a)
        if self._live:
            o = self.optimizer
            self.snaps.append((self._model.store.flat_p.clone(), o.m.clone(), o.v.clone(), o.step_count))


def test_window_of_three_and_a_window_cut_short_by_the_epoch(hip, world, plain_grads, launched_head):
    from reftr_amd.engine_vg import train_one_epoch, train_step
    from reftr_amd.util.misc import NestedTensor
    # three micro-batches, one update
    model, crit, opt = build(world)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=100)
    for i, (s, tg) in enumerate(world["cuda"][:3]):
        gn = train_step(model, crit, s, tg, opt, sched, max_norm=0.1, accum_steps=3)[3]
        assert (gn is None) == (i < 2) and opt.step_count == (1 if i == 2 else 0) and sched.last_epoch == (1 if i == 2 else 0)
    mean = (plain_grads[0] + plain_grads[1] + plain_grads[2]) / 3
    g_rel = rel(model.store.flat_g, mean)
    want = float(mean.double().norm())
    print(f"\n[accum eager k=3] flat_g rel {g_rel:.2e}  grad norm rel {abs(float(gn) - want) / want:.2e}")
    assert g_rel < 1e-6 and abs(float(gn) - want) < 1e-4 * want
    # five batches in windows of two: 2 + 2 + 1
    model, crit, opt = build(world)
    # train_one_epoch switches the model to train(), and some of its dropout sites have a fixed p = 0.1: this instance's train() is
    # pinned to eval mode, so that dropout stays off as in the other comparisons
    model.train = lambda mode=True: model
    sched = _SnapLR(opt, model)
    loader = []
    for samples, targets in world["cpu"]:
        s = {k: v for k, v in samples.items() if k not in ("img", "img_mask")}
        s["img"] = NestedTensor(samples["img"], samples["img_mask"])
        loader.append((s, targets))
    stats = train_one_epoch(model, crit, loader, opt, sched, torch.device("cuda"), 0, max_norm=0.1, accum_steps=2)
    torch.cuda.synchronize()
    assert opt.step_count == 3 and int(opt.step_dev) == 3 and sched.last_epoch == 3 and len(sched.snaps) == 3
    assert [sn[3] for sn in sched.snaps] == [1, 2, 3] and opt.accum_count == 0
    assert stats["loss"] > 0 and stats["grad_norm"] > 0 and not model.training
    caps = model._captured_steps                           # the loop replayed forward + backward from one graph without optimizer nodes
    assert len(caps) == 1 and all(c.accumulate and c.g_opt is None for c in caps.values())
    # the last window holds one batch (s = 1): its update is a plain step on that batch from the state the second update left
    p2, m2, v2, _ = sched.snaps[1]
    ref_model, ref_crit, ref_opt = build(world)
    ref_model.store.flat_p.copy_(p2); ref_opt.m.copy_(m2); ref_opt.v.copy_(v2)
    ref_opt.step_count = 2; ref_opt.step_dev.fill_(2)
    ref_model.mark_dirty(full=True)
    s4, t4 = world["cuda"][4]
    train_step(ref_model, ref_crit, s4, t4, ref_opt, None, max_norm=0.1)
    torch.cuda.synchronize()
    p_rel = rel(model.store.flat_p, ref_model.store.flat_p)
    print(f"[accum epoch 2+2+1] last update vs plain step: flat_p rel {p_rel:.2e}")
    assert p_rel < 1e-7
    assert not torch.equal(sched.snaps[2][0], p2)


def test_captured_windows_match_eager(hip, world, launched_head):
    from reftr_amd.engine_vg import captured_train_step, train_step
    runs = {}
    for mode in ("eager", "graph"):
        model, crit, opt = build(world)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=100)
        p0 = model.store.flat_p.clone()
        losses = []
        for i in range(4):
            s, tg = world["cuda"][i]
            before = model.store.flat_p.clone()
            fn = train_step if mode == "eager" else captured_train_step
            lv, _, _, gn = fn(model, crit, s, tg, opt, sched, max_norm=0.1, accum_steps=2)
            torch.cuda.synchronize()
            losses.append(lv)
            if i % 2 == 0:
                # no update -- deferred or not -- between the micro-batches of a window; the capture's warm-up left no trace either
                assert gn is None and torch.equal(model.store.flat_p, before) and opt.step_count == i // 2
                if i == 0:
                    assert torch.equal(model.store.flat_p, p0) and not opt.m.any() and not opt.v.any() and int(opt.step_dev) == 0
            else:
                assert float(gn) > 0 and not torch.equal(model.store.flat_p, before)
        if mode == "graph":
            caps = model._captured_steps
            assert len(caps) == 1 and all(c.accumulate and c.g_opt is None and not c.deferred for c in caps.values())
            for c in caps.values():
                c.flush()
        assert opt.step_count == 2 and int(opt.step_dev) == 2 and sched.last_epoch == 2
        runs[mode] = (losses, model.store.flat_p.clone(), opt.m.clone(), opt.v.clone())
    (l0, p_e, m_e, v_e), (l1, p_g, m_g, v_g) = runs["eager"], runs["graph"]
    print("\n[accum graph vs eager] loss rel", ["%.1e" % (abs(a - b) / abs(a)) for a, b in zip(l0, l1)],
          f" flat_p {rel(p_g, p_e):.2e}  m {rel(m_g, m_e):.2e}  v {rel(v_g, v_e):.2e}")
    for a, b in zip(l0, l1):
        assert abs(a - b) < 1e-6 * abs(a), (l0, l1)
    assert rel(p_g, p_e) < 1e-7
    assert rel(m_g, m_e) < 1e-6 and rel(v_g, v_e) < 1e-6


def test_accum_steps_one_is_the_plain_step(hip, world, launched_head):
    from reftr_amd.engine_vg import train_step
    s, tg = world["cuda"][0]
    res = []
    for kw in ({}, {"accum_steps": 1}):
        model, crit, opt = build(world)
        lv, _, _, gn = train_step(model, crit, s, tg, opt, None, max_norm=0.1, **kw)
        torch.cuda.synchronize()
        assert opt.accum is None and opt._accum_ws is None and opt.accum_count == 0         # nothing was allocated
        res.append((lv, opt.step_count, int(opt.step_dev), float(gn), model.store.flat_p.clone()))
    a, b = res
    assert a[0] == b[0] and a[1] == b[1] == 1 and a[2] == b[2] == 1
    assert abs(a[3] - b[3]) < 1e-5 * a[3]
    assert rel(b[4], a[4]) < 1e-7


def _free_port():
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); p = sk.getsockname()[1]; sk.close()
    return p


def test_refusals(hip, world, monkeypatch, launched_head):
    import torch.distributed as dist
    from reftr_amd.engine_vg import captured_train_step, train_step
    from reftr_amd.parallel import DistributedDataParallel
    s, tg = world["cuda"][0]
    # a checkpoint inside a window
    model, crit, opt = build(world)
    train_step(model, crit, s, tg, opt, None, max_norm=0.1, accum_steps=2)
    with pytest.raises(RuntimeError, match="accumulation window"):
        opt.state_dict()
    # the data-parallel wrapper
    monkeypatch.setenv("REFTR_DDP_FORCE", "1")
    monkeypatch.setenv("REFTR_DDP_DTYPE", "fp32")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", world_size=1, rank=0)
    try:
        model, crit, opt = build(world)
        runner = DistributedDataParallel(model)
        assert runner.active and model.dp_mode
        p0 = model.store.flat_p.clone()
        for fn in (train_step, captured_train_step):
            with pytest.raises(NotImplementedError, match="data-parallel"):
                fn(runner, crit, s, tg, opt, None, max_norm=0.1, accum_steps=2)
        assert opt.accum is None and opt.step_count == 0 and torch.equal(model.store.flat_p, p0)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
