"""GPU: engine_vg.evaluate(canvas=...) -- every batch of a ragged validation set replayed from one captured graph -- against (1) the
untouched evaluate() where every batch already holds a canvas-sized image, and (2) the composition of the existing public pieces on
the host-padded batch (BatchCanvas.pad_on_host -> model -> criterion -> hip.mask_postprocess with the canvas as frame ->
EvalMeter.update with the un-padded targets -> PostProcessVGMultiPhrase scaled to the original size).

Every comparison is exact (== on python numbers, NaN in the same places): the forward and the loss kernels have no atomics, the
metric counts are integers, the box arithmetic is un-fused fp32 and the running sums add in one order.
"""
import math
import os

import pytest
import torch

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state
from reftr_amd.data.canvas import BatchCanvas

pytestmark = pytest.mark.gpu

SIX = [(128, 128), (96, 128), (128, 96), (64, 96), (112, 80), (80, 112)]


def _build(masks, dec_layers=2):
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase, CriterionVGOnePhraseSeg
    from reftr_amd.models.reftr_transformer import RefTR
    if masks:
        ocfg = O.Cfg(enc_layers=2, dec_layers=dec_layers, bert=O.BertCfg(layers=2), masks=True, aux_loss=False)
        cfg = L.ModelConfig(enc_layers=2, dec_layers=dec_layers, bert=L.BertConfig(layers=2), masks=True)
        model = RefTR(cfg, device="cuda", aux_loss=False)
        crit = CriterionVGOnePhraseSeg(O.weight_dict(ocfg), ["masks", "boxes"])
    else:
        ocfg = O.Cfg(enc_layers=2, dec_layers=dec_layers, bert=O.BertCfg(layers=2))
        cfg = L.ModelConfig(enc_layers=2, dec_layers=dec_layers, bert=L.BertConfig(layers=2))
        model = RefTR(cfg, device="cuda")
        crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
    model.load_state_dict(formula_state(param_shapes(ocfg)), strict=True)
    return model, crit


def _post(masks):
    from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase
    return {"bbox": PostProcessVGMultiPhrase(), "segm": PostProcessSegm()} if masks else {"bbox": PostProcessVGMultiPhrase()}


def make_batch(sizes, j, counts=None, masks=False, n_phrase=3):
    """A CPU loader batch of len(sizes) images padded to their largest (the reference's collate): image b is valid inside sizes[b].
    REC (n_phrase > 0): counts[b] target boxes AND valid phrases on image b.  RES (masks): one box and a [1, h, w] bool mask each."""
    from reftr_amd.util.misc import NestedTensor
    B = len(sizes)
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    n_phrase = 0 if masks else n_phrase
    samples, _ = make_inputs("eval_canvas", B=B, H=H, W=W, L=12, n_phrase=n_phrase)
    img, pad = samples["img"] * (1.0 - 0.05 * j), torch.ones(B, H, W, dtype=torch.bool)
    for b, (h, w) in enumerate(sizes):
        pad[b, :h, :w] = False
    img = img * (~pad)[:, None].float()
    counts = [1] * B if masks else counts
    if n_phrase:
        for k in ("phrase", "phrase_mask", "phrase_pos_l", "phrase_pos_r"):
            samples[k][1:] = samples[k][0]                       # image 0's phrases are all valid
        for b, n in enumerate(counts):
            samples["phrase"][b, n:] = 0; samples["phrase"][b, n:, 0] = 101; samples["phrase"][b, n:, 1] = 102
            samples["phrase_mask"][b, n:] = 0; samples["phrase_mask"][b, n:, :2] = 1
            samples["phrase_pos_l"][b, n:] = 0; samples["phrase_pos_r"][b, n:] = 1
    s = {k: v for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(img, pad)
    gen = torch.Generator().manual_seed(100 * j + H + W)
    targets = []
    for b, ((h, w), n) in enumerate(zip(sizes, counts)):
        u = torch.rand(n, 4, generator=gen)
        t = {"boxes": torch.cat([0.3 + 0.4 * u[:, :2], 0.1 + 0.4 * u[:, 2:]], dim=1), "labels": torch.zeros(n, dtype=torch.long),
             "size": torch.tensor([h, w]), "orig_size": torch.tensor([2 * h + 1, 3 * w]), "image_id": torch.tensor(100 * j + b)}
        if masks:
            t["masks"] = torch.rand(1, h, w, generator=gen) < 0.4
        targets.append(t)
    return s, targets


def ragged(h, w):
    """The two sizes of a batch padded to h x w: the full frame and make_inputs' smaller image."""
    return [(h, w), ((h * 3) // 4, (w * 2) // 3)]


def _cuda(s, t):
    from reftr_amd.engine_vg import _to_device
    return _to_device(s, t, torch.device("cuda"), non_blocking=False)


def compose(model, crit, post, loader, cv, fits=None):
    """evaluate()'s result from the existing public pieces, batch by batch: on the host-padded batch with the canvas as the mask frame
    where the batch goes through the canvas, at its own shape with its own frame where it does not."""
    from reftr_amd import hip
    from reftr_amd.metrics import EvalMeter
    from reftr_amd.util import misc as utils
    model.eval(); crit.eval()
    board, meter, results = utils.StatBoard(), EvalMeter("cuda", seg="segm" in post), {}
    wd = crit.weight_dict
    with torch.no_grad():
        for i, (s, t) in enumerate(loader):
            s, t = _cuda(s, t)
            on = fits is None or fits[i]
            ps, pt = cv.pad_on_host(s, t) if on else (s, t)
            out = model(ps)
            ld = crit(out, pt)
            names = sorted(ld)
            wn = [k for k in names if k in wd]
            un = torch.stack([ld[k].reshape(()).float() for k in names])
            sc = torch.stack([ld[k].reshape(()).float() for k in wn]) * torch.tensor([wd[k] for k in wn], dtype=torch.float32, device="cuda")
            board.add_device([f"{k}_unscaled" for k in names] + wn + ["loss"], torch.cat([un, sc, sc.sum().reshape(1)]))
            orig = torch.stack([x["orig_size" if "orig_size" in t[0] else "size"] for x in t])
            scaled = post["bbox"](out, orig, scale_to_original_shape=True)
            if "segm" in post:
                sizes = [[int(a), int(b)] for a, b in torch.stack([x["size"] for x in t]).tolist()]
                frame_hw = (cv.height, cv.width) if on else (max(a for a, _ in sizes), max(b for _, b in sizes))
                frame, _ = hip.mask_postprocess(out["pred_masks"].squeeze(2).float().contiguous(),
                                                torch.tensor(sizes, dtype=torch.int32).cuda(), frame_hw, post["segm"].threshold)
                meter.update(out, t, masks=frame, sizes=sizes)
            else:
                meter.update(out, t)
            for x, r in zip(t, scaled):
                assert x["boxes"].shape[0] == r["boxes"].shape[0]
                results[int(x["image_id"])] = r["boxes"].cpu().numpy().tolist()
    stats = board.global_avg()
    stats.update(meter.compute())
    return {k: v for k, v in stats.items() if k.split("_")[-1] not in ("unscaled", "0", "1", "2")}, results


def same(a, b):
    """Two stats dicts: the same keys, every value equal, NaN where the other has NaN."""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


@pytest.fixture()
def counted(monkeypatch):
    """Counts the captures of evaluation steps and the calls of the per-shape forward path."""
    import reftr_amd.engine_vg as E
    n = {"captures": 0, "forward_path": 0}
    init, call = E.CapturedEvalStep.__init__, E.CapturedForward.__call__

    def counting_init(self, *a, **kw):
        n["captures"] += 1
        init(self, *a, **kw)

    def counting_call(self, *a, **kw):
        n["forward_path"] += 1
        return call(self, *a, **kw)
    monkeypatch.setattr(E.CapturedEvalStep, "__init__", counting_init)
    monkeypatch.setattr(E.CapturedForward, "__call__", counting_call)
    return n


def test_canvas_sized_image_in_every_batch_equals_evaluate(hip, counted):
    """REC+RES, canvas 128 x 128: every batch holds a 128 x 128 image beside a smaller one, so the untouched evaluate() pads to the
    canvas by itself and its mask frame is the canvas: evaluate(canvas=cv) must return its stats and results, key for key."""
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks=True)
    post = _post(True)
    loader = [make_batch([(128, 128), small], j, masks=True) for j, small in enumerate([(64, 96), (96, 64), (80, 112)])]
    want, res_want = evaluate(model, crit, post, loader, torch.device("cuda"))
    assert counted["captures"] == 0
    got, res_got = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=BatchCanvas(128, 128, 1, masks=True))
    same(got, want)
    assert res_got == res_want and list(res_got) == list(res_want) == [0, 1, 100, 101, 200, 201]
    assert counted["captures"] == 1 and got["seg_miou"] > 0 and math.isfinite(got["loss"])


@pytest.mark.parametrize("masks", [False, True], ids=["rec", "rec_res"])
def test_six_shapes_one_capture_against_the_composition(hip, counted, capfd, masks):
    """Six batches of six shapes.  REC: three phrase slots, box counts varying per image, one image with none.  One capture, made once,
    and no batch on the per-shape forward path."""
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks)
    post = _post(masks)
    counts = [(3, 2), (1, 3), (2, 0), (3, 1), (2, 3), (1, 2)]
    loader = [make_batch(ragged(h, w), j, counts=counts[j], masks=masks) for j, (h, w) in enumerate(SIX)]
    cv = BatchCanvas(128, 128, 1 if masks else 3, masks=masks)
    want, res_want = compose(model, crit, post, loader, cv)
    capfd.readouterr()
    before = counted["forward_path"]
    got, res_got = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=cv)
    err = capfd.readouterr().err
    assert "does not fit" not in err and "ignored" not in err, err
    same(got, want)
    assert res_got == res_want and list(res_got) == list(res_want) and len(res_got) == 12
    assert counted["captures"] == 1 and counted["forward_path"] == before
    if not masks:
        assert res_got[201] == [] and [len(res_got[k]) for k in (0, 1, 100, 101)] == [3, 2, 1, 3]


def test_largest_first_and_smallest_first_agree(hip):
    """Any stale byte of the previous batch in a static buffer shows when a small batch follows a large one.  Each order equals its own
    composition; the two orders equal each other too: the double sums add four fp32 values each, which is exact in double whatever the
    order, the other totals are integers."""
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks=True)
    post = _post(True)
    big, small = make_batch(ragged(128, 128), 0, masks=True), make_batch(ragged(64, 96), 1, masks=True)
    cv = BatchCanvas(128, 128, 1, masks=True)
    runs = []
    for loader in ([big, small], [small, big]):
        got, res = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=cv)
        want, res_want = compose(model, crit, post, loader, cv)
        same(got, want)
        assert res == res_want
        runs.append((got, res))
    same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]


def test_misfits_in_the_middle_take_the_existing_path(hip, counted, capfd):
    """An image larger than the canvas and a batch with more boxes than the capacity between fitting batches: one stderr line per
    reason, the same totals and results in loader order, and the fitting batch after them replays the one capture."""
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks=False)
    post = _post(False)
    loader = [make_batch(ragged(96, 128), 0, counts=(2, 1)), make_batch(ragged(160, 128), 1, counts=(1, 2)),
              make_batch(ragged(128, 96), 2, counts=(1, 2)), make_batch(ragged(64, 96), 3, counts=(3, 1)),
              make_batch(ragged(64, 96), 4, counts=(2, 2)), make_batch(ragged(160, 128), 5, counts=(2, 1))]
    cv = BatchCanvas(128, 128, 2)
    fits = [True, False, True, False, True, False]
    assert [cv.fits(*b) for b in loader] == fits
    want, res_want = compose(model, crit, post, loader, cv, fits=fits)
    capfd.readouterr()
    got, res_got = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=cv)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if "does not fit" in ln]
    assert len(lines) == 2 and "exceeds the canvas" in lines[0] and "capacity 2" in lines[1], err
    same(got, want)
    assert res_got == res_want and list(res_got) == list(res_want)
    assert counted["captures"] == 1 and counted["forward_path"] == 3


def rec_res_misfit_loader():
    """REC+RES, B = 2, for a 128 x 128 masks=True canvas: fits, an image larger than the canvas, fits, `orig_size` missing on one image
    (a misfit by why_not_eval; image 0, so that the path at the batch's own shape scales every box by `size`)."""
    loader = [make_batch(ragged(h, w), j, masks=True) for j, (h, w) in enumerate([(96, 128), (160, 128), (64, 96), (128, 96)])]
    del loader[3][1][0]["orig_size"]
    return loader


def test_rec_res_misfits_alternate_with_canvas_batches(hip, counted, capfd):
    """The REC+RES twin of the test above: the meter's two producers (rt_eval_canvas inside the replayed graph, EvalMeter.update) and the
    segmentation frame (the canvas, the batch's own) alternate batch by batch; totals, results and their order are the composition's."""
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks=True)
    post = _post(True)
    loader = rec_res_misfit_loader()
    cv = BatchCanvas(128, 128, 1, masks=True)
    fits = [True, False, True, False]
    assert [cv.why_not(*b) is None and cv.why_not_eval(*b, segm=True) is None for b in loader] == fits
    want, res_want = compose(model, crit, post, loader, cv, fits=fits)
    capfd.readouterr()
    got, res_got = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=cv)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "does not fit" in ln]
    assert len(lines) == 2 and "exceeds the canvas" in lines[0] and "orig_size" in lines[1], lines
    same(got, want)
    assert res_got == res_want and list(res_got) == list(res_want) == [0, 1, 100, 101, 200, 201, 300, 301]
    assert counted["captures"] == 1 and counted["forward_path"] == 2 and got["seg_miou"] > 0


def test_refusals_and_switches(hip, monkeypatch, counted):
    from reftr_amd.engine_vg import evaluate
    model, crit = _build(masks=False)
    post = _post(False)
    loader = [make_batch(ragged(96, 128), 0, counts=(3, 2))] * 2
    cv = BatchCanvas(128, 128, 3)
    dev = torch.device("cuda")
    with pytest.raises(NotImplementedError, match="visualize"):
        evaluate(model, crit, post, loader, dev, visualize=True, canvas=cv)
    assert counted["captures"] == 0 and counted["forward_path"] == 0           # refused before anything was launched
    plain = evaluate(model, crit, post, loader, dev)
    again = evaluate(model, crit, post, loader, dev, canvas=None)
    same(plain[0], again[0])
    assert plain[1] == again[1]
    for switch in ("REFTR_EVAL_METRICS", "REFTR_EVAL_GRAPH"):
        monkeypatch.setenv(switch, "0")
        off = evaluate(model, crit, post, loader, dev)
        off_cv = evaluate(model, crit, post, loader, dev, canvas=cv)
        monkeypatch.delenv(switch)
        same(off[0], off_cv[0])
        assert off[1] == off_cv[1] and counted["captures"] == 0
    on = evaluate(model, crit, post, loader, dev, canvas=cv)
    # switched back on: captured (the values are another batch's -- 96 x 128 padded to the canvas -- and are held by the tests above)
    assert counted["captures"] == 1 and list(on[1]) == list(plain[1]) and sorted(on[0]) == sorted(plain[0])


@pytest.fixture
def coop_env(hip):
    """Restores what a forced failure changes for the whole process: the poll budget and the REFTR_DEC_COOP* switches."""
    import reftr_amd.engine_vg as E
    saved = {k: os.environ.get(k) for k in ("REFTR_DEC_COOP", "REFTR_DEC_COOP_BWD")}
    logged = E._COOP_LOGGED
    try:
        yield hip
    finally:
        hip.decoder_set_spin(0)
        E._COOP_LOGGED = logged
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_failsafe_counts_every_batch_once(coop_env, counted):
    """The cooperative decoder's hand-off forced to time out (a poll budget of 1, as tests/test_failsafe_gpu.py forces it): the first
    replay's results are vetoed on the device, the loop falls back to the launched chain and runs the batch again -- the stats are the
    chain's, with every image counted once."""
    from reftr_amd.engine_vg import evaluate
    hip = coop_env
    post = _post(False)
    loader = [make_batch([(96, 128), (72, 85), (96, 128), (72, 85)], 0, n_phrase=0, counts=[1] * 4),
              make_batch([(64, 96), (48, 64), (64, 96), (48, 64)], 1, n_phrase=0, counts=[1] * 4)]
    cv = BatchCanvas(96, 128, 1)
    ref_model, crit = _build(masks=False, dec_layers=3)
    ref_model.net.dec_coop = ref_model.net.dec_coop_bwd = False
    want, res_want = compose(ref_model, crit, post, loader, cv)
    model, crit = _build(masks=False, dec_layers=3)
    assert model.net.dec_coop and model.net.dec_stack_coop_ok(4, 1, 24, 3, True)
    hip.decoder_set_spin(1)
    got, res_got = evaluate(model, crit, post, loader, torch.device("cuda"), canvas=cv)
    assert os.environ.get("REFTR_DEC_COOP") == "0" and not model.net.dec_coop          # the fall-back happened
    same(got, want)
    assert res_got == res_want and len(res_got) == 8
    assert counted["captures"] == 2                                                    # the vetoed capture and the chain's
