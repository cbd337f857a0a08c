"""GPU: training steps on RAW batches (reftr_amd.data.RawImages: uint8 images of any sizes, pixel boxes) through the batch canvas.

A raw batch's step IS the existing step on BatchCanvas.pad_on_host of it (the DeviceInputPipeline chain, then the canvas's padding);
rt_raw_stage delivers the same bytes (tests/test_raw_stage_gpu.py), so the buffers of the capture are compared byte for byte and the
steps with the eager-vs-graph gates of tests/test_canvas_step_gpu.py, whose tiny model, token fields and gates are reused: B = 2,
canvas 128 x 128, three box slots, eval mode.  Raw sources at size 96 / max_size 128: 72 x 96 and 90 x 90, 150 x 100 and 48 x 64,
64 x 200 and 128 x 96, 96 x 128 (identity) and 33 x 41 -- four batches, four pairs of sizes, four box-count patterns."""
import pytest
import torch

from reftr_amd.data import RawImages
from reftr_amd.data.canvas import BatchCanvas
from test_canvas_step_gpu import build, flush, hand_over, launched_head, make_batch, same_step, state_of  # noqa: F401
from test_canvas_step_gpu import world  # noqa: F401

pytestmark = pytest.mark.gpu

RAW = [(((72, 96), (90, 90)), (3, 2)), (((150, 100), (48, 64)), (1, 3)), (((64, 200), (128, 96)), (2, 2)), (((96, 128), (33, 41)), (3, 1))]


def raw_batch(sizes, counts, j, size=96, max_size=128, L=12, n_phrase=3):
    """The token fields and box counts of test_canvas_step_gpu.make_batch, with raw uint8 images and xyxy pixel boxes."""
    samples, targets = make_batch((32, 32), counts, j, L=L, n_phrase=n_phrase)
    gen = torch.Generator().manual_seed(7 + j)
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = RawImages([torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).cuda() for h, w in sizes], size, max_size)
    t = []
    for (h, w), tg in zip(sizes, targets):
        cx, cy, bw, bh = tg["boxes"].unbind(-1)
        xyxy = torch.stack([(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h], dim=-1)
        t.append({"boxes": xyxy.cuda(), "labels": tg["labels"].cuda()})
    return s, t


def buffers(staged):
    return [staged.samples["img"].tensors.view(torch.int32), staged.samples["img"].mask.view(torch.uint8),
            staged.targets_static[0].view(torch.int32), staged.targets_static[1], staged.targets_static[2].view(torch.int32)]


def test_four_raw_batches_one_graph(hip, world, launched_head, capfd):
    from reftr_amd.engine_vg import captured_train_step, train_step
    cv = BatchCanvas(128, 128, 3)
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    batches = [raw_batch(sizes, counts, j) for j, (sizes, counts) in enumerate(RAW)]
    assert len({tuple(b[0]["img"].out_sizes()) for b in batches}) == 4 and len({cv.key(b[0]) for b in batches}) == 1
    capfd.readouterr()
    for i, (s, t) in enumerate(batches):
        assert cv.fits(s, t)
        hand_over(state_of(model, opt), twin, topt)
        got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
        flush(model)
        assert len(model._captured_steps) == 1
        cap, = model._captured_steps.values()
        ps, pt = cv.pad_on_host(s, t)
        want_staged = cv.stage(ps, pt)
        torch.cuda.synchronize()
        for a, b in zip(buffers(cap.staged), buffers(want_staged)):
            assert torch.equal(a, b), i                          # the capture's buffers: the bytes of the existing chain
        for k, v in s.items():
            if torch.is_tensor(v):
                assert torch.equal(cap.staged.samples[k], v), k
        want = train_step(twin, tcrit, ps, pt, topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        same_step(got, want, model, twin, f"raw graph {i}")
    assert cap.canvas is cv and cap.key == cv.key(batches[0][0]) and opt.step_count == 4
    assert "does not fit" not in capfd.readouterr().err


def test_eager_raw_step_and_lookahead_staging(hip, world, launched_head):
    """train_step(canvas=) on a raw batch, and begin_train_step staging the NEXT raw batch under the running replay."""
    from reftr_amd.engine_vg import Lookahead, captured_train_step, train_step
    cv = BatchCanvas(128, 128, 3)
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    batches = [raw_batch(sizes, counts, j) for j, (sizes, counts) in enumerate(RAW[:3])]
    hand_over(state_of(model, opt), twin, topt)
    got = train_step(model, crit, *batches[0], opt, None, max_norm=0.1, canvas=cv)
    want = train_step(twin, tcrit, *cv.pad_on_host(*batches[0]), topt, None, max_norm=0.1)
    torch.cuda.synchronize()
    same_step(got, want, model, twin, "raw eager")
    assert crit.targets_static is None
    for k in (1, 2):
        hand_over(state_of(model, opt), twin, topt)
        nxt = batches[2] if k == 1 else None
        got = captured_train_step(model, crit, *batches[k], opt, None, max_norm=0.1, canvas=cv, lookahead=Lookahead(lambda n=nxt: n))
        if k == 1:
            cap, = model._captured_steps.values()
            assert cap._staged is not None and cap._staged[0] is batches[2][0]        # staged under the replay
        flush(model)
        want = train_step(twin, tcrit, *cv.pad_on_host(*batches[k]), topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        same_step(got, want, model, twin, f"raw lookahead {k}")
    assert len(model._captured_steps) == 1


def test_misfit_raw_batch_runs_at_its_own_shape(hip, world, launched_head, capfd):
    """96 x 160 at size 96 / max_size 160 stays 96 x 160: wider than the canvas.  It is resized by the existing chain and runs as
    that NestedTensor batch runs without a canvas; said once, although it comes twice."""
    from reftr_amd.engine_vg import captured_train_step, train_step
    cv = BatchCanvas(128, 128, 3)
    model, crit, opt = build(world)
    twin, tcrit, topt = build(world)
    s, t = raw_batch(((96, 160), (80, 100)), (3, 2), 5, size=96, max_size=160)
    assert s["img"].out_sizes() == [(96, 160), (96, 120)] and "exceeds the canvas" in cv.why_not(s, t)
    capfd.readouterr()
    for visit in range(2):
        hand_over(state_of(model, opt), twin, topt)
        got = captured_train_step(model, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
        flush(model)
        ns, nt = cv.resized(s, t)
        assert tuple(ns["img"].tensors.shape) == (2, 3, 96, 160)
        want = train_step(twin, tcrit, ns, nt, topt, None, max_norm=0.1)
        torch.cuda.synchronize()
        same_step(got, want, model, twin, f"raw misfit {visit}")
    err = capfd.readouterr().err
    assert err.count("does not fit") == 1 and "exceeds the canvas" in err, err
    (key, cap), = model._captured_steps.items()
    assert cap.canvas is None and tuple(cap.s["img"].tensors.shape) == (2, 3, 96, 160)       # captured at its own shape


def test_refusals(hip, world, launched_head):
    from reftr_amd.engine_vg import captured_train_step, evaluate, train_one_epoch, train_step
    from reftr_amd.models.post_process import PostProcessVGMultiPhrase
    from reftr_amd.parallel import DistributedDataParallel
    cv = BatchCanvas(128, 128, 3)
    model, crit, opt = build(world)
    p0 = model.store.flat_p.clone()
    s, t = raw_batch(*RAW[0], 0)
    host = ({k: v.to("cpu") for k, v in s.items()}, [{k: v.to("cpu") for k, v in tg.items()} for tg in t])
    for fn in (train_step, captured_train_step):                                       # a raw batch without a canvas
        with pytest.raises(NotImplementedError, match="needs canvas="):
            fn(model, crit, s, t, opt, None, max_norm=0.1)
    with pytest.raises(NotImplementedError, match="needs canvas="):
        train_one_epoch(model, crit, [host], opt, None, torch.device("cuda"), 0, max_norm=0.1)
    model.eval()
    for canvas in (None, cv):                                                          # evaluate
        with pytest.raises(NotImplementedError, match="raw batch"):
            evaluate(model, crit, {"bbox": PostProcessVGMultiPhrase()}, [host], torch.device("cuda"), canvas=canvas)
    runner = DistributedDataParallel(model)                                            # under the data-parallel wrapper
    for fn in (train_step, captured_train_step):
        with pytest.raises(NotImplementedError, match="data-parallel"):
            fn(runner, crit, s, t, opt, None, max_norm=0.1, canvas=cv)
    torch.cuda.synchronize()
    assert opt.step_count == 0 and torch.equal(model.store.flat_p, p0) and not getattr(model, "_captured_steps", None)
