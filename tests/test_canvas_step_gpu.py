"""GPU: training steps through the batch canvas against the existing code's step on the host-padded batch.

A canvas step IS the existing step at the canvas's shape (BatchCanvas.pad_on_host is the definition, rt_batch_stage delivers the same
bytes -- tests/test_batch_stage_gpu.py), so the gates are the project's eager-vs-graph gates (tests/test_grad_accum_gpu.py, from
tests/test_backbone_variants_gpu.py): flat_g rel-L2 < 1e-6, gradient norm < 1e-4, weights < 1e-7, loss entries to a relative 1e-6.
Only the 4 % of the gradient buffer that backward accumulates with atomics keeps them from being bit gates.

Tiny model (one bottleneck per ResNet stage, 2 encoder / decoder / BERT layers) in eval mode: dropout off.  Batches: B = 2, L = 12,
three phrase slots, images 96 x 128, 128 x 96, 64 x 128 and 128 x 128, box counts permuted between batches; canvas (128, 128) with
three boxes per image.
"""
import numpy as np
import pytest
import torch

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state
from reftr_amd.data.canvas import BatchCanvas

pytestmark = pytest.mark.gpu

LAYERS = (1, 1, 1, 1)
# (an image without any valid phrase is outside the model's domain -- every query masked, NaN gradients in the existing step as in the
# reference, tests/test_edge_cases_gpu.py -- so every image keeps at least one box here; the count 0 is the kernel test's)
SHAPES = [((96, 128), (3, 2)), ((128, 96), (1, 3)), ((64, 128), (2, 2)), ((128, 128), (3, 1)), ((96, 96), (2, 3)), ((64, 96), (1, 2))]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def make_batch(hw, counts, j=0, L=12, n_phrase=3, mask_hw=None, name="canvas_step"):
    """A make_inputs batch whose image b has counts[b] target boxes AND counts[b] valid phrases (the criterion pairs them); the
    other phrase slots hold the empty phrase.  With mask_hw: one box per image and a [1, h, w] target mask each (RES)."""
    samples, targets = make_inputs(name, B=len(counts), H=hw[0], W=hw[1], L=L, n_phrase=n_phrase)
    samples["img"] = samples["img"] * (1.0 - 0.05 * j)
    gen = torch.Generator().manual_seed(100 * j + hw[0] + hw[1])
    if n_phrase:
        for k in ("phrase", "phrase_mask", "phrase_pos_l", "phrase_pos_r"):
            samples[k][1:] = samples[k][0]                       # image 0's phrases are all valid
        for b, n in enumerate(counts):
            samples["phrase"][b, n:] = 0; samples["phrase"][b, n:, 0] = 101; samples["phrase"][b, n:, 1] = 102
            samples["phrase_mask"][b, n:] = 0; samples["phrase_mask"][b, n:, :2] = 1
            samples["phrase_pos_l"][b, n:] = 0; samples["phrase_pos_r"][b, n:] = 1
    out = []
    for b, n in enumerate(counts):
        u = torch.rand(n, 4, generator=gen)
        t = {"boxes": torch.cat([0.3 + 0.4 * u[:, :2], 0.1 + 0.4 * u[:, 2:]], dim=1), "labels": torch.zeros(n, dtype=torch.long)}
        if mask_hw is not None:
            t["masks"] = torch.rand(1, *mask_hw[b], generator=gen) < 0.4
        out.append(t)
    return samples, out


def nested(samples, targets, device=None):
    from reftr_amd.util.misc import NestedTensor
    mv = (lambda v: v.to(device)) if device else (lambda v: v)
    s = {k: mv(v) for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(mv(samples["img"]), mv(samples["img_mask"]))
    return s, [{k: mv(v) for k, v in t.items()} for t in targets]


@pytest.fixture(scope="module")
def world():
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), resnet_layers=LAYERS)
    raw = [make_batch(hw, counts, j) for j, (hw, counts) in enumerate(SHAPES)]
    return {"ocfg": ocfg, "P": formula_state(param_shapes(ocfg)), "cpu": [nested(*b) for b in raw], "cuda": [nested(*b, device="cuda") for b in raw]}


def build(world):
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


def canvas():
    return BatchCanvas(128, 128, 3)


def flush(model):
    for c in model._captured_steps.values():
        c.flush()
    torch.cuda.synchronize()


def state_of(model, opt):
    """(weights, moments, update count) with nothing pending."""
    flush(model) if model.__dict__.get("_captured_steps") else torch.cuda.synchronize()
    return model.store.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.step_count


def hand_over(state, twin, topt):
    """The twin takes the state the model had in front of its step: every step is compared FROM EQUAL WEIGHTS.  (Two runs of the
    existing eager loop on this model part ways by themselves -- flat_p 4e-5 after six steps, from the atomics' 2e-10 after the first,
    about x 300 per Adam step -- so a chain of steps can only be held update by update.)"""
    twin.store.flat_p.copy_(state[0]); topt.m.copy_(state[1]); topt.v.copy_(state[2])
    topt.step_count = state[3]; topt.step_dev.fill_(state[3])
    twin.mark_dirty(full=True)


def same_step(got, want, model, twin, what):
    """(loss_value, scaled, unscaled, grad norm) and the weights of `model` against the existing step's on `twin`."""
    val = lambda v: float(v.detach()) if torch.is_tensor(v) else float(v)      # noqa: E731
    lv, gn, un = got[0], val(got[3]), {k: val(v) for k, v in got[2].items()}
    lv0, gn0, un0 = want[0], val(want[3]), {k: val(v) for k, v in want[2].items()}
    assert sorted(un) == sorted(un0)
    worst = max(abs(float(un[k]) - float(un0[k])) / max(abs(float(un0[k])), 1e-30) for k in un0)
    n_rel = abs(float(gn) - float(gn0)) / float(gn0)
    p_rel = rel(model.store.flat_p, twin.store.flat_p)
    print(f"\n[{what}] loss entries rel {worst:.1e}  total rel {abs(lv - lv0) / abs(lv0):.1e}  grad norm rel {n_rel:.1e}  flat_p rel {p_rel:.1e}")
    assert np.isfinite(lv) and lv > 0
    assert worst < 1e-6 and abs(lv - lv0) < 1e-6 * abs(lv0)
    assert n_rel < 1e-4
    assert p_rel < 1e-7


def test_eager_step_on_the_canvas_is_the_step_on_the_padded_batch(hip, world, launched_head):
    from reftr_amd.engine_vg import train_step
    cv = canvas()
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    p0 = model.store.flat_p.clone()
    for i, (s, t) in enumerate(world["cuda"][:4]):
        # from equal weights: the twin's state is handed over before every step
        model.store.flat_p.copy_(twin.store.flat_p); opt.m.copy_(topt.m); opt.v.copy_(topt.v); model.mark_dirty(full=True)
        got = train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
        want = train_step(twin, tcrit, *cv.pad_on_host(s, t), topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        g_rel = rel(model.store.flat_g, twin.store.flat_g)
        print(f"\n[canvas eager {i}] flat_g rel {g_rel:.1e}")
        assert g_rel < 1e-6
        same_step(got, want, model, twin, f"canvas eager {i}")
        assert crit.targets_static is None and crit.target_masks_static is None
    assert not torch.equal(model.store.flat_p, p0) and opt.step_count == 4
    assert not crit._off_cache and not crit._nb_cache              # the host-built offsets / counts were never consulted


def test_four_shapes_one_graph(hip, world, launched_head):
    """Four batches of four image shapes and four box-count patterns replay ONE capture.  On the parent commit (no canvas) the same
    four batches create four captures -- every one of them is a shape key of its own -- and a fifth shape runs eagerly."""
    from reftr_amd.engine_vg import CapturedTrainStep, captured_train_step, train_step
    cv = canvas()
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    assert len({CapturedTrainStep.shape_key(s, t) for s, t in world["cuda"][:4]}) == 4
    for i, (s, t) in enumerate(world["cuda"][:4]):
        hand_over(state_of(model, opt), twin, topt)
        got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
        flush(model)
        want = train_step(twin, tcrit, *cv.pad_on_host(s, t), topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        same_step(got, want, model, twin, f"canvas graph {i}")
        assert len(model._captured_steps) == 1
    cap, = model._captured_steps.values()
    assert cap.canvas is cv and cap.key == cv.key(world["cuda"][0][0]) and opt.step_count == 4
    assert tuple(cap.s["img"].tensors.shape) == (2, 3, 128, 128)
    assert not crit._off_cache and not crit._nb_cache and crit.targets_static is None


def test_largest_then_smallest_through_the_replay(hip, world, launched_head):
    """Stale state: the buffers of the capture held a canvas-sized image and six boxes before the smallest batch arrives."""
    from reftr_amd.engine_vg import captured_train_step
    cv = canvas()
    big = nested(*make_batch((128, 128), (3, 3), j=7), device="cuda")
    small = nested(*make_batch((64, 96), (1, 1), j=8), device="cuda")
    model, crit, opt = build(world)
    captured_train_step(model, crit, *big, opt, None, max_norm=0.1, canvas=cv)
    flush(model)
    state = (model.store.flat_p.clone(), opt.m.clone(), opt.v.clone())
    got = captured_train_step(model, crit, *small, opt, None, max_norm=0.1, canvas=cv)
    flush(model)
    assert len(model._captured_steps) == 1
    fresh, fcrit, fopt = build(world)
    fresh.store.flat_p.copy_(state[0]); fopt.m.copy_(state[1]); fopt.v.copy_(state[2])
    fopt.step_count = 1; fopt.step_dev.fill_(1)
    fresh.mark_dirty(full=True)
    want = captured_train_step(fresh, fcrit, *small, fopt, None, max_norm=0.1, canvas=cv)
    flush(fresh)
    same_step(got, want, model, fresh, "canvas stale")


def _pin_eval(model):
    # train_one_epoch switches the model to train(), and some dropout sites have a fixed p: this instance stays in eval mode
    model.train = lambda mode=True: model


class _SnapLR(torch.optim.lr_scheduler.StepLR):
    """StepLR that keeps (weights, moments) as they are on the stream when the loop steps it -- right behind the launch of replay k,
    whose head applied update k - 1 (the deferred schedule): the state IN FRONT of update k."""

    def __init__(self, opt, model):
        self.snaps, self._model, self._live = [], model, False
        super().__init__(opt, step_size=100)
        self._live = True

    def step(self, *a):
        super().step(*a)
        if self._live:
            o = self.optimizer
            self.snaps.append((self._model.store.flat_p.clone(), o.m.clone(), o.v.clone(), len(self.snaps)))


def test_epoch_of_six_shapes_is_one_capture(hip, world, launched_head, capfd):
    """train_one_epoch(canvas=...) over six batches of six shapes: one capture, no fallback, and every one of its six updates --
    five applied inside the next replay, the last by the flush -- is the existing eager step on the host-padded batch from the state
    the loop had in front of it (weights rel-L2 < 1e-7, as tests/test_grad_accum_gpu.py holds its epoch loop).  The end-to-end
    distance to an eager loop run beside it is printed: the existing eager loop does not reproduce ITSELF to 1e-7 over six steps on
    this model (see hand_over)."""
    from reftr_amd.engine_vg import train_one_epoch, train_step
    cv = canvas()
    model, crit, opt = build(world)
    _pin_eval(model)
    sched = _SnapLR(opt, model)
    assert all(cv.fits(s, t) for s, t in world["cpu"]) and len(world["cpu"]) == 6
    capfd.readouterr()
    stats = train_one_epoch(model, crit, world["cpu"], opt, sched, torch.device("cuda"), 0, max_norm=0.1, canvas=cv)
    flush(model)
    err = capfd.readouterr().err
    assert "does not fit" not in err and "eagerly" not in err, err           # no batch fell back
    assert len(model._captured_steps) == 1 and opt.step_count == 6 and int(opt.step_dev) == 6 and sched.last_epoch == 6
    assert stats["loss"] > 0 and stats["grad_norm"] > 0 and len(sched.snaps) == 6
    after = [sn[0] for sn in sched.snaps[1:]] + [model.store.flat_p.clone()]
    after_m = [sn[1] for sn in sched.snaps[1:]] + [opt.m.clone()]
    assert not torch.equal(after[0], sched.snaps[0][0]) and not torch.equal(after[5], after[4])
    twin, tcrit, topt = build(world)
    worst = 0.0
    for k, (s, t) in enumerate(world["cuda"]):
        hand_over(sched.snaps[k], twin, topt)
        train_step(twin, tcrit, *cv.pad_on_host(s, t), topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        p_rel, m_rel = rel(after[k], twin.store.flat_p), rel(after_m[k], topt.m)
        worst = max(worst, p_rel)
        assert p_rel < 1e-7 and m_rel < 1e-6, (k, p_rel, m_rel)
    chain, ccrit, copt = build(world)
    for s, t in world["cuda"]:
        train_step(chain, ccrit, *cv.pad_on_host(s, t), copt, None, max_norm=0.1)
    torch.cuda.synchronize()
    print(f"\n[canvas epoch] worst update flat_p rel {worst:.1e}; end to end against an eager loop {rel(model.store.flat_p, chain.store.flat_p):.1e}")


def test_accumulation_on_the_canvas(hip, world, launched_head):
    from reftr_amd.engine_vg import captured_train_step, train_step
    cv = canvas()
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    for i, (s, t) in enumerate(world["cuda"][:4]):
        if i % 2 == 0:
            hand_over(state_of(model, opt), twin, topt)
        got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, accum_steps=2, canvas=cv)
        want = train_step(twin, tcrit, *cv.pad_on_host(s, t), topt, None, max_norm=0.1, accum_steps=2)
        torch.cuda.synchronize()
        assert (got[3] is None) == (want[3] is None) == (i % 2 == 0)
        assert abs(got[0] - want[0]) < 1e-6 * abs(want[0])
        if i % 2:
            same_step(got, want, model, twin, f"canvas accumulate {i}")
    caps = model._captured_steps
    assert len(caps) == 1 and all(c.accumulate and c.g_opt is None and c.canvas is cv for c in caps.values())
    assert opt.step_count == 2 and int(opt.step_dev) == 2 and opt.accum_count == 0


def test_res_target_masks_of_two_sizes(hip, launched_head):
    from reftr_amd.engine_vg import captured_train_step, train_step
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGOnePhraseSeg
    from reftr_amd.models.reftr_transformer import RefTR
    from reftr_amd.optim import FusedAdamW
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), masks=True, aux_loss=False)
    P = formula_state(param_shapes(ocfg))

    def build_seg():
        cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), masks=True)
        model = RefTR(cfg, device="cuda", aux_loss=False)
        model.load_state_dict(P, strict=True)
        model.eval()
        return model, CriterionVGOnePhraseSeg(O.weight_dict(ocfg), ["masks", "boxes"]), FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)

    cv = BatchCanvas(128, 128, 1, masks=True)
    batches = [nested(*make_batch((96, 128), (1, 1), j=0, n_phrase=0, mask_hw=[(96, 128), (72, 85)], name="canvas_seg"), device="cuda"),
               nested(*make_batch((128, 96), (1, 1), j=1, n_phrase=0, mask_hw=[(100, 64), (128, 96)], name="canvas_seg"), device="cuda")]
    model, crit, opt = build_seg()
    twin, tcrit, topt = build_seg()
    p0 = model.store.flat_p.clone()

    def rewind(m, o):
        # back to the initial weights and optimizer state (as tests/test_seg_gpu.py::test_cem_training_steps_captured restores them)
        for c in m.__dict__.get("_captured_steps", {}).values():
            c.reset_pending()
        m.store.flat_p.copy_(p0); o.m.zero_(); o.v.zero_(); o.step_dev.zero_(); o.step_count = 0
        m.mark_dirty(full=True)

    for i, (s, t) in enumerate(batches):
        # Both steps start from the initial weights: a second step from once-updated weights is outside what two eager runs of this
        # fixture reproduce (the mask head's GroupNorm + ReLU stages amplify the first step's atomics noise; see hand_over and
        # tests/test_seg_gpu.py::test_cem_training_steps_captured).  The forward has no atomics, so from equal weights every loss
        # entry is held at the relative 1e-6 and the gradient norm at 1e-4.
        rewind(model, opt); rewind(twin, topt)
        got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
        flush(model)
        want = train_step(twin, tcrit, *cv.pad_on_host(s, t), topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        for k in sorted(want[2]):
            a, b = float(got[2][k]), float(want[2][k].detach())
            assert b > 0 and abs(a - b) < 1e-6 * abs(b), (k, got[2], want[2])
        assert {"loss_mask_unscaled", "loss_dice_unscaled"} <= set(want[2])
        gn, gn0 = float(got[3]), float(want[3])
        print(f"\n[canvas RES {i}] grad norm rel {abs(gn - gn0) / gn0:.1e}  flat_p rel {rel(model.store.flat_p, twin.store.flat_p):.1e}")
        assert abs(gn - gn0) < 1e-4 * gn0
    assert len(model._captured_steps) == 1
    cap, = model._captured_steps.values()
    assert tuple(cap.staged.tgt_masks.shape) == (2, 1, 128, 128) and crit.target_masks_static is None


def test_batches_that_do_not_fit_take_the_existing_path(hip, world, launched_head, capfd):
    """A 160-pixel-wide image, four boxes on an image, L = 10: each runs exactly as without a canvas -- at its own shape, under
    `max_shapes` -- and the canvas capture replays the next fitting batch.  max_shapes = 1 here: the canvas capture holds the one
    slot, so the three shapes take the eager step (test_misfit_captured_at_its_own_shape: the captured route)."""
    from reftr_amd.engine_vg import captured_train_step, train_step
    cv = canvas()
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    s0, t0 = world["cuda"][0]
    hand_over(state_of(model, opt), twin, topt)
    got = captured_train_step(model, crit, s0, t0, opt, None, max_norm=0.1, max_shapes=1, canvas=cv)
    flush(model)
    want = train_step(twin, tcrit, *cv.pad_on_host(s0, t0), topt, None, max_norm=0.1)
    same_step(got, want, model, twin, "canvas fit 0")
    misfits = [("wide", nested(*make_batch((96, 160), (3, 2), j=3), device="cuda")),
               ("boxes", nested(*make_batch((96, 128), (4, 1), j=4, n_phrase=4), device="cuda")),
               ("tokens", nested(*make_batch((96, 128), (3, 2), j=5, L=10), device="cuda"))]
    capfd.readouterr()
    for what, (s, t) in misfits:
        assert not cv.fits(s, t)
        for _ in range(2 if what == "wide" else 1):                # the second visit of a shape says nothing
            hand_over(state_of(model, opt), twin, topt)
            got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, max_shapes=1, canvas=cv)
            flush(model)
            want = train_step(twin, tcrit, s, t, topt, None, max_norm=0.1)       # the existing result, at the batch's own shape
            torch.cuda.synchronize()
            same_step(got, want, model, twin, f"canvas misfit {what}")
    err = capfd.readouterr().err
    assert err.count("does not fit") == 3 and "exceeds the canvas" in err and "token field shapes" in err, err
    (key, cap), = model._captured_steps.items()                    # the canvas capture is still there, and alone
    assert key[0][0] == "canvas" and cap.canvas is cv and tuple(cap.s["img"].tensors.shape) == (2, 3, 128, 128)
    s1, t1 = world["cuda"][1]
    hand_over(state_of(model, opt), twin, topt)
    got = captured_train_step(model, crit, s1, t1, opt, None, max_norm=0.1, max_shapes=1, canvas=cv)
    flush(model)
    want = train_step(twin, tcrit, *cv.pad_on_host(s1, t1), topt, None, max_norm=0.1)
    same_step(got, want, model, twin, "canvas fit 1 after the misfits")
    assert len(model._captured_steps) == 1 and opt.step_count == 6


def test_misfit_captured_at_its_own_shape(hip, world, launched_head):
    """Default max_shapes: a 160-pixel-wide batch is captured at its own shape beside the canvas capture (CapturedTrainStep without
    a canvas from begin_train_step(canvas=...)), visited twice, with look-ahead staging across the two captures; each step is then
    repeated by the existing eager step from the state the model had in front of it.  The twin runs AFTER the model's sequence."""
    from reftr_amd.engine_vg import Lookahead, captured_train_step, train_step
    cv = canvas()
    model, crit, opt = build(world)
    wide = nested(*make_batch((96, 160), (3, 2), j=3), device="cuda")
    seq = [world["cuda"][0], wide, wide, world["cuda"][1], world["cuda"][2]]
    states, gots = [], []
    for k, (s, t) in enumerate(seq):
        states.append(state_of(model, opt))
        nxt = seq[k + 1] if k + 1 < len(seq) else None
        gots.append(captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv, lookahead=Lookahead(lambda n=nxt: n)))
    final = state_of(model, opt)
    keys = [k[0] for k in model._captured_steps]
    assert len(keys) == 2 and sum(k[0] == "canvas" for k in keys) == 1
    assert [c.canvas is cv for c in model._captured_steps.values()].count(True) == 1
    twin, tcrit, topt = build(world)
    for k, (s, t) in enumerate(seq):
        hand_over(states[k], twin, topt)
        ps, pt = cv.pad_on_host(s, t) if cv.fits(s, t) else (s, t)
        want = train_step(twin, tcrit, ps, pt, topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        nxt_p = states[k + 1][0] if k + 1 < len(seq) else final[0]
        lv, gn = gots[k][0], float(gots[k][3])
        p_rel = rel(nxt_p, twin.store.flat_p)
        print(f"\n[canvas + own-shape capture {k}] loss rel {abs(lv - want[0]) / want[0]:.1e}  grad norm rel {abs(gn - float(want[3])) / float(want[3]):.1e}  flat_p rel {p_rel:.1e}")
        assert abs(lv - want[0]) < 1e-6 * want[0] and abs(gn - float(want[3])) < 1e-4 * float(want[3]) and p_rel < 1e-7


def test_fused_head_on_the_canvas(hip, world):
    """The production default (REFTR_HEAD_FUSE on: rt_head_loss reads boxes, offsets and count from targets_static, zero-padded tail
    included): a canvas replay of the smallest batch after the largest against the existing fused replay -- no canvas -- of the
    host-padded batch on a fresh model with the same weights."""
    import os
    from reftr_amd.engine_vg import captured_train_step
    assert os.environ.get("REFTR_HEAD_FUSE", "1") != "0"
    cv = canvas()
    big = nested(*make_batch((128, 128), (3, 3), j=7), device="cuda")
    small = nested(*make_batch((64, 96), (1, 2), j=8), device="cuda")
    model, crit, opt = build(world)
    captured_train_step(model, crit, *big, opt, None, max_norm=0.1, canvas=cv)
    state = state_of(model, opt)
    got = captured_train_step(model, crit, *small, opt, None, max_norm=0.1, canvas=cv)
    flush(model)
    cap, = model._captured_steps.values()
    assert cap.canvas is cv and cap._direct_loss_ok()                                          # the direct path, fused head
    fresh, fcrit, fopt = build(world)
    hand_over(state, fresh, fopt)
    want = captured_train_step(fresh, fcrit, *cv.pad_on_host(*small), fopt, None, max_norm=0.1)
    flush(fresh)
    assert next(iter(fresh._captured_steps.values())).canvas is None
    same_step(got, want, model, fresh, "canvas fused head")


def test_data_parallel_wrapper_refuses_the_canvas(hip, world, launched_head):
    from reftr_amd.engine_vg import captured_train_step, train_one_epoch, train_step
    from reftr_amd.parallel import DistributedDataParallel
    cv = canvas()
    model, crit, opt = build(world)
    runner = DistributedDataParallel(model)
    p0 = model.store.flat_p.clone()
    s, t = world["cuda"][0]
    for fn in (train_step, captured_train_step):
        for kw in ({}, {"accum_steps": 2}):
            with pytest.raises(NotImplementedError, match="data-parallel"):
                fn(runner, crit, s, t, opt, None, max_norm=0.1, canvas=cv, **kw)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        train_one_epoch(runner, crit, [world["cpu"][0]], opt, None, torch.device("cuda"), 0, max_norm=0.1, canvas=cv)
    torch.cuda.synchronize()
    assert opt.step_count == 0 and torch.equal(model.store.flat_p, p0) and not getattr(model, "_captured_steps", None)
