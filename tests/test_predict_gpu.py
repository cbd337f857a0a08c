"""GPU: reftr_amd.Predictor -- raw batches replayed from one captured graph (forward -> rt_predict_canvas) -- against the definition
of a prediction computed eagerly from the existing public pieces: BatchCanvas.pad_on_host -> the model in eval mode ->
hip.box_postprocess scaled to the raw sizes -> masks_origin of hip.mask_postprocess with the canvas as its frame.

Every comparison is exact: the forward has no atomics and the tail's two kernels are held bit for bit in test_predict_kernel_gpu.py.
"""
import os

import pytest
import torch

from reftr_amd.data import RawImages
from reftr_amd.data.canvas import BatchCanvas
from test_eval_canvas_gpu import _build, _post, coop_env, make_batch  # noqa: F401
from test_predict_kernel_gpu import oracle_masks

pytestmark = pytest.mark.gpu

RAW = [((72, 96), (90, 90)), ((150, 100), (48, 64)), ((64, 200), (128, 96))]


def raw_samples(sizes, j, counts=None, masks=False, n_phrase=3, size=96, max_size=128, device="cuda"):
    """The token fields of test_eval_canvas_gpu.make_batch with raw uint8 images of `sizes`."""
    B = len(sizes)
    s, _ = make_batch([(32, 32)] * B, j, counts=counts if counts is not None else [1] * B, masks=masks, n_phrase=n_phrase)
    gen = torch.Generator().manual_seed(17 + j)
    s = {k: v.to(device) for k, v in s.items() if k != "img"}
    s["img"] = RawImages([torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).to(device) for h, w in sizes], size, max_size)
    return s


def no_targets(B):
    return [{"boxes": torch.zeros((0, 4), device="cuda")} for _ in range(B)]


def origs_of(s):
    return [(int(im.shape[0]), int(im.shape[1])) for im in s["img"].images]


def definition(hip, model, post, cv, s):
    """What a prediction is, eagerly, from the existing public pieces."""
    model.eval()
    B, origs = len(s["img"]), origs_of(s)
    with torch.no_grad():
        ps, _ = cv.pad_on_host(s, no_targets(B))
        out = model(ps)
        pb = out["pred_boxes"].to(torch.float32).contiguous()
        _, P, K, _ = pb.shape
        xyxy, counts = hip.box_postprocess(pb, out["phrase_mask"].reshape(B, P, K).to(torch.uint8).contiguous(),
                                           torch.tensor(origs, dtype=torch.float32).cuda())
        res = [{"boxes": xyxy[b, :n].cpu()} for b, n in enumerate(counts.tolist())]
        if "segm" in post:
            pm = out["pred_masks"]
            pm = (pm.squeeze(2) if pm.dim() == 5 else pm).to(torch.float32).contiguous()
            blocks = oracle_masks(hip, pm, s["img"].out_sizes(), origs, (cv.height, cv.width), post["segm"].threshold)
            for r, blk, (oh, ow) in zip(res, blocks, origs):
                r["masks"] = blk.view(pm.shape[1], 1, oh, ow).cpu()
    return res


def same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        assert g["boxes"].dtype == torch.float32 and g["boxes"].shape == w["boxes"].shape and not g["boxes"].is_cuda
        assert torch.equal(g["boxes"].view(torch.int32), w["boxes"].view(torch.int32))
        if "masks" in w:
            assert g["masks"].dtype == torch.uint8 and g["masks"].shape == w["masks"].shape and torch.equal(g["masks"], w["masks"])


@pytest.fixture()
def counted(monkeypatch, hip):
    """The ABI calls the host issues (by name, in order) and the captures of prediction steps."""
    import reftr_amd.predict as PR
    n = {"calls": [], "captures": 0}
    call, init = hip._call, PR._PredictStep.__init__

    def counting_call(name, *a, **kw):
        n["calls"].append(name)
        return call(name, *a, **kw)

    def counting_init(self, *a, **kw):
        n["captures"] += 1
        init(self, *a, **kw)
    monkeypatch.setattr(hip, "_call", counting_call)
    monkeypatch.setattr(PR._PredictStep, "__init__", counting_init)
    return n


@pytest.mark.parametrize("masks", [False, True], ids=["rec", "rec_res"])
def test_three_raw_batches_one_capture(hip, counted, capfd, masks):
    """Three raw batches of different image sizes (the third from host memory): boxes and masks equal the definition exactly, from ONE
    capture; after it the host issues two ABI calls per batch -- rt_raw_stage and rt_predict_facts -- and a replay."""
    from reftr_amd import Predictor
    model, _ = _build(masks)
    post = _post(masks)
    cv = BatchCanvas(128, 128, 1 if masks else 3)
    counts = [(3, 2), (0, 3), (1, 2)]
    batches = [raw_samples(sizes, j, counts=counts[j], masks=masks, device="cpu" if j == 2 else "cuda") for j, sizes in enumerate(RAW)]
    assert len({tuple(b["img"].out_sizes()) for b in batches}) == 3
    p = Predictor(model, post, cv, max_orig_size=(160, 200))
    capfd.readouterr()
    for j, s in enumerate(batches):
        model.train()                                                                 # (definition() below leaves it in eval mode)
        counted["calls"].clear()
        got = p(s)
        issued = list(counted["calls"])
        assert model.training                                                         # the caller's mode is back
        assert all(not t.is_cuda for r in got for t in r.values())
        if masks:
            assert [tuple(r["masks"].shape) for r in got] == [(1, 1, h, w) for h, w in RAW[j]]
        else:
            assert all("masks" not in r for r in got)
            assert [r["boxes"].shape[0] for r in got] == list(counts[j])
        got = [{k: v.clone() for k, v in r.items()} for r in got]                      # (valid until the next call)
        on_dev = {k: (v.to("cuda") if hasattr(v, "to") else v) for k, v in s.items()}
        want = definition(hip, model, post, cv, on_dev)
        same_results(got, want)
        if j > 0:
            assert issued == ["rt_raw_stage", "rt_predict_facts"], issued
    assert counted["captures"] == 1 and len(p.steps) == 1
    assert "does not fit" not in capfd.readouterr().err
    if masks:
        assert any(0 < int(r["masks"].sum()) < r["masks"].numel() for r in got)


def test_misfit_runs_the_chain_at_its_own_shape(hip, counted, capfd):
    """96 x 160 at size 96 / max_size 160 stays 96 x 160: wider than the canvas.  The batch equals the existing chain at its own shape
    (BatchCanvas.resized -> the model -> the two post-processors); said once, although it comes twice."""
    from reftr_amd import Predictor
    model, _ = _build(True)
    post = _post(True)
    cv = BatchCanvas(128, 128, 1)
    s = raw_samples([(96, 160), (80, 100)], 5, masks=True, size=96, max_size=160)
    p = Predictor(model, post, cv, max_orig_size=(160, 200))
    assert s["img"].out_sizes() == [(96, 160), (96, 120)] and "exceeds the canvas" in p.why_not(s)
    model.eval()
    origs = torch.tensor(origs_of(s))
    with torch.no_grad():
        ns, nt = cv.resized(s, no_targets(2))
        assert tuple(ns["img"].tensors.shape) == (2, 3, 96, 160)
        out = model(ns)
        boxes = post["bbox"](out, origs, scale_to_original_shape=True)
        segm = post["segm"]([{} for _ in nt], out, origs, torch.stack([t["size"] for t in nt]))
        want = [{"boxes": b["boxes"].cpu(), "masks": m["masks_origin"].cpu()} for b, m in zip(boxes, segm)]
    capfd.readouterr()
    for visit in range(2):
        got = p(s)
        same_results(got, want)
        assert [tuple(r["masks"].shape) for r in got] == [(1, 1, 96, 160), (1, 1, 80, 100)]
    err = capfd.readouterr().err
    assert err.count("does not fit") == 1 and "exceeds the canvas" in err, err
    assert counted["captures"] == 0 and not p.steps and not model.training
    big = raw_samples([(72, 96), (161, 100)], 6, masks=True, size=48, max_size=64)     # fits the canvas, not max_orig_size
    assert "exceeds max_orig_size 160 x 200" in p.why_not(big)
    got = p(big)
    assert [tuple(r["masks"].shape) for r in got] == [(1, 1, 72, 96), (1, 1, 161, 100)] and counted["captures"] == 0


def test_refusals(hip):
    from reftr_amd import Predictor
    from reftr_amd.parallel import DistributedDataParallel
    from reftr_amd.util.misc import NestedTensor
    model, _ = _build(False)
    cv = BatchCanvas(128, 128, 3)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        Predictor(DistributedDataParallel(model), _post(False), cv, max_orig_size=(160, 200))
    with pytest.raises(NotImplementedError, match="post-processor"):
        Predictor(model, {"bbox": torch.nn.Identity()}, cv, max_orig_size=(160, 200))
    p = Predictor(model, _post(False), cv, max_orig_size=(160, 200))
    s = raw_samples(RAW[0], 0, counts=(3, 2))
    nested = dict(s, img=NestedTensor(torch.zeros(2, 3, 96, 128, device="cuda"), torch.zeros(2, 96, 128, dtype=torch.bool, device="cuda")))
    model.train()
    with pytest.raises(TypeError, match="RawImages"):
        p(nested)
    assert model.training and not p.steps


def test_failsafe_returns_the_chains_results(coop_env, counted):
    """The cooperative decoder's hand-off forced to time out exactly as tests/test_eval_canvas_gpu.py forces it (a poll budget of 1):
    the failure word is read after the batch, the capture is dropped, and the batch runs again on the launched chain -- the results
    are the chain's."""
    from reftr_amd import Predictor
    hip = coop_env
    post = _post(False)
    cv = BatchCanvas(96, 128, 1)
    batches = [raw_samples([(72, 96), (90, 90), (48, 64), (45, 60)], 0, n_phrase=0), raw_samples([(36, 48), (96, 128), (50, 50), (72, 96)], 1, n_phrase=0)]
    ref_model, _ = _build(masks=False, dec_layers=3)
    ref_model.net.dec_coop = ref_model.net.dec_coop_bwd = False
    want = [definition(hip, ref_model, post, cv, s) for s in batches]
    model, _ = _build(masks=False, dec_layers=3)
    assert model.net.dec_coop and model.net.dec_stack_coop_ok(4, 1, 24, 3, True)
    p = Predictor(model, post, cv, max_orig_size=(128, 128))
    hip.decoder_set_spin(1)
    for s, w in zip(batches, want):
        same_results(p(s), w)
    assert os.environ.get("REFTR_DEC_COOP") == "0" and not model.net.dec_coop          # the fall-back happened
    assert counted["captures"] == 2 and len(p.steps) == 1                              # the dropped capture and the chain's
