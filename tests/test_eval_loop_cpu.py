"""CPU: engine_vg.evaluate()'s loop on stubs -- the reference's per-image torch path end to end, the canvas switches and refusals,
the run-again-on-the-launched-chain helper and the loader-order merge of the results.  The model, the criterion and the box
post-processor are stubs in plain torch (the package's own need the HIP library); every expectation is recomputed here from the
stub's outputs with util.box_ops and compared with ==.
"""
import numpy as np
import pytest
import torch
from torch import nn

from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.metrics import decode_ring
from reftr_amd.util.box_ops import box_cxcywh_to_xyxy, box_iou
from test_eval_canvas_gpu import make_batch, ragged

P = 3
COUNTS = [(3, 2), (1, 3)]
WEIGHTS = {"loss_bbox": 5.0, "loss_giou": 2.0, "loss_giou_0": 2.0}         # an aux weight without a loss, as with aux_loss=False


def _outputs(j, B):
    g = torch.Generator().manual_seed(1000 + j)
    u = torch.rand(B, P, 1, 4, generator=g)
    boxes = torch.cat([0.3 + 0.4 * u[..., :2], 0.1 + 0.5 * u[..., 2:]], dim=-1)
    valid = torch.stack([torch.arange(P) < n for n in COUNTS[j]])
    return {"pred_boxes": boxes, "phrase_mask": valid}


class StubModel(nn.Module):
    """pred_boxes [B, P, 1, 4] and phrase_mask [B, P] of loader batch `calls % 2`, from a generator seeded by the batch."""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, samples):
        j = self.calls % len(COUNTS)
        self.calls += 1
        return _outputs(j, samples["img"].tensors.shape[0])


class StubCriterion(nn.Module):
    weight_dict = WEIGHTS

    def forward(self, outputs, targets):
        pred = torch.cat([outputs["pred_boxes"][b, :len(t["boxes"]), 0] for b, t in enumerate(targets)])
        return {"loss_bbox": (pred - torch.cat([t["boxes"] for t in targets])).abs().mean(), "loss_giou": outputs["pred_boxes"].mean()}


class TorchBoxPost:
    """PostProcessVGMultiPhrase's contract in plain torch: the valid phrases' boxes as xyxy, scaled by (w, h, w, h) on request."""

    def __call__(self, outputs, target_sizes, scale_to_original_shape=False):
        boxes = box_cxcywh_to_xyxy(outputs["pred_boxes"][:, :, 0])
        if scale_to_original_shape:
            h, w = target_sizes.unbind(1)
            boxes = boxes * torch.stack([w, h, w, h], dim=1).to(torch.float32)[:, None]
        return [{"boxes": boxes[b][outputs["phrase_mask"][b].bool()]} for b in range(len(boxes))]


def _loader():
    loader = [make_batch(ragged(96, 128), 0, counts=COUNTS[0]), make_batch(ragged(64, 96), 1, counts=COUNTS[1])]
    del loader[1][1][0]["image_id"]
    return loader


def _expected(loader):
    hit = total = torch.zeros(())
    cnt, vecs, results = 0, [], {}
    for j, (samples, targets) in enumerate(loader):
        out = _outputs(j, len(targets))
        ld = StubCriterion()(out, targets)
        sc = torch.stack([ld["loss_bbox"].float(), ld["loss_giou"].float()]) * torch.tensor([5.0, 2.0])
        vecs.append(torch.cat([sc, sc.sum().reshape(1)]).to(torch.float64))
        for b, t in enumerate(targets):
            n = len(t["boxes"])
            xyxy = box_cxcywh_to_xyxy(out["pred_boxes"][b, :n, 0])
            iou = torch.diag(box_iou(box_cxcywh_to_xyxy(t["boxes"]), xyxy)[0])
            hit = hit + (iou > 0.5).float().sum(); total = total + iou.sum(); cnt += n
            if "image_id" in t:
                oh, ow = t["orig_size"].tolist()
                results[int(t["image_id"])] = (xyxy * torch.tensor([ow, oh, ow, oh], dtype=torch.float32)).tolist()
    means = ((vecs[0] + vecs[1]) / 2).tolist()
    stats = {"loss_bbox": means[0], "loss_giou": means[1], "loss": means[2],
             "accuracy_iou0.5": float(hit / cnt), "miou": float(total / cnt)}
    return stats, results


def test_reference_path_on_the_cpu():
    from reftr_amd.engine_vg import evaluate
    loader = _loader()
    model = StubModel()
    stats, results = evaluate(model, StubCriterion(), {"bbox": TorchBoxPost()}, loader, torch.device("cpu"))
    want, res_want = _expected(loader)
    assert model.calls == 2 and not model.training
    assert stats == want and sorted(stats) == sorted(want)
    assert not any(k.split("_")[-1] in ("unscaled", "0", "1", "2") for k in stats)
    assert list(results) == [0, 1, 101] and 100 not in results                   # loader order; the image without an id is absent
    assert results == res_want
    assert [len(results[k]) for k in (0, 1, 101)] == [3, 2, 3]
    assert all(type(r) is list and len(r) == 4 and all(type(v) is float for v in r) for rows in results.values() for r in rows)
    assert 0.0 < stats["miou"] < 1.0


def test_switches_and_refusals_on_the_cpu(capfd):
    from reftr_amd.engine_vg import evaluate
    loader, post, dev = _loader(), {"bbox": TorchBoxPost()}, torch.device("cpu")
    cv = BatchCanvas(128, 128, 3)
    plain = evaluate(StubModel(), StubCriterion(), post, loader, dev)
    model = StubModel()
    capfd.readouterr()
    first = evaluate(model, StubCriterion(), post, loader, dev, canvas=cv)
    again = evaluate(model, StubCriterion(), post, loader, dev, canvas=cv)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "ignored" in ln]
    assert len(lines) == 1 and "a CPU device" in lines[0] and repr(cv) in lines[0], lines            # said once per model
    assert first == plain and again == plain and list(first[1]) == list(plain[1])
    calls = model.calls
    with pytest.raises(NotImplementedError, match="visualize"):
        evaluate(model, StubCriterion(), post, loader, dev, visualize=True, canvas=cv)
    assert model.calls == calls                                                                      # refused before the model ran


def _patched_failures(monkeypatch, failures):
    import reftr_amd.engine_vg as E
    log = []
    monkeypatch.setattr(E, "_cooperative_failed", lambda model: bool(failures and failures.pop(0)))
    monkeypatch.setattr(E, "_coop_fallback", lambda model: log.append("fallback"))
    return E, log


@pytest.mark.parametrize("failures", [[True], [True, True]], ids=["fails_once", "fails_twice"])
def test_run_again_runs_twice_at_most(monkeypatch, failures):
    E, log = _patched_failures(monkeypatch, list(failures))
    out = E._run_again_on_chain(object(), lambda: log.append("run") or len(log), drop=lambda: log.append("drop"))
    assert log == ["run", "fallback", "drop", "run"] and out == 4            # the second run's value; a second failure is not asked for
    log.clear()
    E._run_again_on_chain(object(), lambda: log.append("run"))                # no hook: nothing of the caller's to drop
    assert log == (["run"] if len(failures) == 1 else ["run", "fallback", "run"])


def test_run_again_without_a_failure_runs_once(monkeypatch):
    E, log = _patched_failures(monkeypatch, [])
    assert E._run_again_on_chain(object(), lambda: log.append("run") or "value", drop=lambda: log.append("drop")) == "value"
    assert log == ["run"]


def test_results_merge_in_loader_order():
    """fits = T, F, T, F, T, F: ring slots and the misfits' own dicts alternate; every image id is the loader's, a misfit's id 21
    is also what the ring holds for a later slot's image -- the later batch's value wins, as in a plain loop -- and a misfit's id
    that no ring names keeps its value."""
    from reftr_amd.engine_vg import _LoaderOrder
    rng = np.random.default_rng(1)
    boxes = rng.uniform(0, 500, size=(4, 2, 3, 4)).astype(np.float32)
    counts = np.array([[2, 1], [3, 0], [1, 1], [0, 0]], dtype=np.int32)
    ids = np.array([[10, 11], [30, 31], [50, 21], [0, 0]], dtype=np.int64)
    order, batches, decoded = _LoaderOrder(), [], []
    misfits = [{20: [[1.0, 2.0, 3.0, 4.0]], 21: []}, {40: [[5.0, 6.0, 7.0, 8.0]]}, {60: [], 10: [[9.0, 9.0, 9.0, 9.0]]}]
    for batch_no in range(6):
        if batch_no % 2 == 0:
            order.slot(decoded, len(batches))
            batches.append((batch_no, True, counts[len(batches)].tolist()))
        else:
            order.fill().update(misfits[batch_no // 2])
    decoded += decode_ring(boxes, counts, ids, 3, 0, batches)                # the ring is read back after the loop
    merged = {}
    order.merge(merged)
    assert list(merged) == [10, 11, 20, 21, 30, 31, 40, 50, 60]
    assert merged[20] == misfits[0][20] and merged[40] == misfits[1][40] and merged[60] == []      # not overwritten by the ring
    assert merged[11] == boxes[0, 1, :1].tolist() and merged[30] == boxes[1, 0, :3].tolist() and merged[31] == []
    assert merged[21] == boxes[2, 1, :1].tolist() and merged[10] == [[9.0, 9.0, 9.0, 9.0]]          # a repeated id: the later batch
