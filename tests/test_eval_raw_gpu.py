"""GPU: engine_vg.evaluate_raw -- raw batches replayed from one captured graph (rt_raw_stage -> forward -> criterion -> rt_eval_canvas ->
rt_eval_orig) -- against its two definitions:
  * the existing keys and results_dict: evaluate(canvas=) on the batches converted by BatchCanvas.resized_eval (the DeviceInputPipeline
    chain, with `size`, `orig_size` and `image_id` as tensors);
  * the '_orig' keys: BatchCanvas.pad_on_host -> the model -> masks_origin of rt_mask_postprocess with the canvas as its frame
    (test_predict_kernel_gpu.oracle_masks), query 0 -> integer counts against the raw mask bytes -> metrics.stats_from_orig_accumulators.

Every comparison is exact (== on python numbers, NaN in the same places).
"""
import pytest
import torch

from reftr_amd.data.canvas import BatchCanvas
from test_eval_canvas_gpu import _build, _post, same
from test_predict_gpu import RAW, origs_of, raw_samples
from test_predict_kernel_gpu import oracle_masks

pytestmark = pytest.mark.gpu

MISFIT = [(96, 160), (80, 100)]           # at size 96 / max_size 160 the first stays 96 x 160: wider than the 128 x 128 canvas
THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


def raw_batch(sizes, j, counts=None, masks=False, ids=True, device="cuda", **kw):
    """A raw evaluation batch: test_predict_gpu.raw_samples + targets in the raw frame (boxes xyxy pixels, counts[b] of them; RES: one
    box and a uint8 [1, h, w] mask with bytes from {0, 1, 2, 255}); no `size`, no `orig_size`."""
    counts = [1] * len(sizes) if masks or counts is None else counts
    s = raw_samples(sizes, j, counts=counts, masks=masks, device=device, **kw)
    gen = torch.Generator().manual_seed(300 + j)
    values = torch.tensor([0, 0, 1, 2, 255], dtype=torch.uint8)
    targets = []
    for b, ((h, w), n) in enumerate(zip(sizes, counts)):
        u = torch.rand(n, 4, generator=gen)
        x0, y0 = 0.5 * w * u[:, 0], 0.5 * h * u[:, 1]
        t = {"boxes": torch.stack([x0, y0, x0 + (0.1 + 0.4 * u[:, 2]) * w, y0 + (0.1 + 0.4 * u[:, 3]) * h], dim=1),
             "labels": torch.zeros(n, dtype=torch.long)}
        if masks:
            t["masks"] = values[torch.randint(0, 5, (1, h, w), generator=gen)]
        if ids:
            t["image_id"] = torch.tensor(100 * j + b)
        targets.append({k: v.to(device) for k, v in t.items()})
    return s, targets


def on_cuda(batch):
    from reftr_amd.engine_vg import _to_device
    return _to_device(*batch, torch.device("cuda"), non_blocking=False)


def orig_definition(hip, model, post, cv, loader, fits):
    """The '_orig' keys by the definition, eagerly: per image integer {I, U} on the raw frame; then the host formulas."""
    from reftr_amd.metrics import stats_from_orig_accumulators
    model.eval()
    n, hits, si, su, total = 0, [0] * 5, 0, 0, 0.0
    with torch.no_grad():
        for batch, fit in zip(loader, fits):
            s, t = on_cuda(batch)
            ps, _ = cv.pad_on_host(s, t) if fit else cv.resized(s, t)
            frame = tuple(ps["img"].tensors.shape[-2:])
            assert frame == (cv.height, cv.width) or not fit
            pm = model(ps)["pred_masks"]
            pm = (pm.squeeze(2) if pm.dim() == 5 else pm).to(torch.float32).contiguous()
            origs = origs_of(s)
            for blk, (oh, ow), tg in zip(oracle_masks(hip, pm, s["img"].out_sizes(), origs, frame, post["segm"].threshold), origs, t):
                pred, tgt = blk[:oh * ow] != 0, tg["masks"].reshape(-1) != 0
                i, u = int((pred & tgt).sum()), int((pred | tgt).sum())
                iou = torch.tensor(i, dtype=torch.float32) / torch.tensor(u, dtype=torch.float32)
                n, si, su, total = n + 1, si + i, su + u, total + float(iou)
                for k, thr in enumerate(THRESHOLDS):
                    hits[k] += int(bool(iou > torch.tensor(thr, dtype=torch.float32)))
    return stats_from_orig_accumulators([n, *hits, si, su, total])


def reference(model, crit, post, cv, loader):
    """The existing keys and results: evaluate(canvas=) on the resized_eval form of the same batches."""
    from reftr_amd.engine_vg import evaluate
    converted = [cv.resized_eval(*on_cuda(b)) for b in loader]
    for s, t in converted:
        assert all(x["size"].dtype == torch.int64 and x["orig_size"].is_cuda for x in t)
    return evaluate(model, crit, post, converted, torch.device("cuda"), canvas=cv)


def split_orig(stats):
    return {k: v for k, v in stats.items() if not k.endswith("_orig")}, {k: v for k, v in stats.items() if k.endswith("_orig")}


class Marked:
    """A loader that notes in `log` where each batch begins."""

    def __init__(self, batches, log):
        self.batches, self.log = batches, log

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for j, b in enumerate(self.batches):
            self.log.append(("batch", j))
            yield b


@pytest.fixture()
def counted(monkeypatch, hip):
    """In order: the ABI calls the host issues (by name), the device-to-host reads (.cpu() / .tolist()), the loader's batch marks;
    and the number of captures."""
    import reftr_amd.engine_vg as E
    n = {"log": [], "captures": 0}
    call, init, cpu, tolist = hip._call, E.CapturedEvalStep.__init__, torch.Tensor.cpu, torch.Tensor.tolist

    def counting_call(name, *a, **kw):
        n["log"].append(name)
        return call(name, *a, **kw)

    def counting_init(self, *a, **kw):
        n["captures"] += 1
        init(self, *a, **kw)

    def counting_cpu(self, *a, **kw):
        if self.is_cuda:
            n["log"].append("to_host")
        return cpu(self, *a, **kw)

    def counting_tolist(self):
        if self.is_cuda:
            n["log"].append("to_host")
        return tolist(self)
    monkeypatch.setattr(hip, "_call", counting_call)
    monkeypatch.setattr(E.CapturedEvalStep, "__init__", counting_init)
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    monkeypatch.setattr(torch.Tensor, "tolist", counting_tolist)
    return n


def per_batch(log):
    """The log cut at the batch marks: [what was issued while batch j was evaluated]."""
    out = []
    for entry in log:
        if isinstance(entry, tuple):
            out.append([])
        elif out:
            out[-1].append(entry)
    return out


def loader_of(masks, misfit=False):
    counts = [(3, 2), (0, 3), (1, 2)]
    batches = [raw_batch(sizes, j, counts=counts[j], masks=masks, device="cpu" if j == 2 else "cuda") for j, sizes in enumerate(RAW)]
    if misfit:
        batches.append(raw_batch(MISFIT, 3, counts=(2, 1), masks=masks, size=96, max_size=160))
    return batches


@pytest.mark.parametrize("masks", [False, True], ids=["rec", "rec_res"])
def test_three_raw_batches_one_capture(hip, counted, capfd, masks):
    """Three raw batches of different image sizes (the third from host memory).  One capture; after it the host issues two ABI calls
    per batch -- rt_raw_stage and rt_eval_raw_facts -- and a replay, and reads nothing back before finish."""
    from reftr_amd import evaluate_raw
    model, crit = _build(masks)
    post = _post(masks)
    cv = BatchCanvas(128, 128, 1 if masks else 3, masks=masks)
    loader = loader_of(masks)
    assert len({tuple(b[0]["img"].out_sizes()) for b in loader}) == 3 and not loader[2][0]["img"].is_cuda
    want, res_want = reference(model, crit, post, cv, loader)
    model.train(); crit.train()
    sentinel = object()
    crit.targets_static = sentinel
    capfd.readouterr()
    counted["log"].clear(); counted["captures"] = 0
    got, res_got = evaluate_raw(model, crit, post, Marked(loader, counted["log"]), torch.device("cuda"), cv)
    issued = per_batch(counted["log"])
    assert "does not fit" not in capfd.readouterr().err
    assert model.training and crit.training and crit.targets_static is sentinel         # modes and the criterion's switch are back
    crit.targets_static = None
    old, new = split_orig(got)
    same(old, want)
    assert res_got == res_want and list(res_got) == list(res_want) == [0, 1, 100, 101, 200, 201]
    assert counted["captures"] == 1
    assert issued[1] == ["rt_raw_stage", "rt_eval_raw_facts"], issued[1]
    assert issued[2][:2] == ["rt_raw_stage", "rt_eval_raw_facts"] and "to_host" in issued[2][2:]       # finish reads back, once
    assert not any(name.startswith("rt_") for name in issued[2][2:]), issued[2]
    if masks:
        same(new, orig_definition(hip, model, post, cv, loader, [True] * 3))
        assert sorted(new) == sorted(["seg_miou_orig", "seg_oiou_orig"] + [f"seg_prec@{t}_orig" for t in THRESHOLDS])
        assert 0.0 < new["seg_oiou_orig"] < 1.0 and new["seg_oiou_orig"] != old["seg_oiou"]   # another frame, another annotation
    else:
        assert new == {} and res_got[100] == [] and [len(res_got[k]) for k in (0, 1, 101)] == [3, 2, 3]


def test_a_misfit_is_converted_once_and_adds_to_the_same_totals(hip, counted, capfd):
    """REC+RES.  The fourth batch holds an image that stays wider than the canvas; it comes twice.  Said once; existing keys, results
    and the '_orig' totals are the definitions' over all five batches, in loader order, and the fitting batches share ONE capture."""
    from reftr_amd import evaluate_raw
    model, crit = _build(True)
    post = _post(True)
    cv = BatchCanvas(128, 128, 1, masks=True)
    loader = loader_of(True, misfit=True)
    loader = loader[:2] + [loader[3]] + loader[2:]                                     # fits, fits, misfit, fits (host), misfit
    fits = [True, True, False, True, False]
    assert [cv.why_not(*b) is None for b in loader] == fits and loader[2][0]["img"].out_sizes() == [(96, 160), (96, 120)]
    want, res_want = reference(model, crit, post, cv, loader)
    capfd.readouterr()
    counted["captures"] = 0
    got, res_got = evaluate_raw(model, crit, post, loader, torch.device("cuda"), cv)
    err = capfd.readouterr().err
    assert err.count("does not fit") == 1 and "exceeds the canvas" in err, err
    old, new = split_orig(got)
    same(old, want)
    assert res_got == res_want and list(res_got) == list(res_want)
    same(new, orig_definition(hip, model, post, cv, loader, fits))
    assert counted["captures"] == 1


def test_ids_on_all_targets_or_on_none(hip, counted):
    """With `image_id` (on the device, on the host) the results are keyed by it; without, the dict is empty and no metric moves."""
    from reftr_amd import evaluate_raw
    model, crit = _build(False)
    post = _post(False)
    cv = BatchCanvas(128, 128, 3)
    counts = [(3, 2), (1, 3)]
    with_ids = [raw_batch(RAW[j], j, counts=counts[j], device="cpu" if j else "cuda") for j in range(2)]
    without = [raw_batch(RAW[j], j, counts=counts[j], ids=False, device="cpu" if j else "cuda") for j in range(2)]
    a, res_a = evaluate_raw(model, crit, post, with_ids, torch.device("cuda"), cv)
    b, res_b = evaluate_raw(model, crit, post, without, torch.device("cuda"), cv)
    same(a, b)
    assert list(res_a) == [0, 1, 100, 101] and [len(res_a[k]) for k in res_a] == [3, 2, 1, 3] and res_b == {}
    some = [(with_ids[0][0], [with_ids[0][1][0], without[0][1][1]])]
    c, res_c = evaluate_raw(model, crit, post, some + with_ids[1:], torch.device("cuda"), cv)     # a misfit by why_not_eval_raw
    # (that batch ran at its own shape, 96 x 128: its boxes are that forward's; the second batch went through the canvas as before)
    assert list(res_c) == [0, 100, 101] and len(res_c[0]) == 3 and res_c[100] == res_a[100] and res_c[101] == res_a[101]
