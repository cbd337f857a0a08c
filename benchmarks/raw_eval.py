"""Validation over RAW batches end to end: engine_vg.evaluate_raw beside the best path the package had for the same data before it.

Data: a validation set of six raw shapes -- uint8 images of {640x640, 480x640, 640x480, 427x640, 512x640, 640x427} (the sizes of
benchmarks/ragged_eval.py; a batch holds B = 8 images of one shape, RawImages(size = the shorter side, max_size = 640): the resize keeps
the size, both paths run Pillow's two resample passes), boxes xyxy in pixels, for REC+RES a uint8 [1, h, w] mask per image, `image_id`;
a seeded shuffle of every block of six.  Batches are seeded and pinned.  Models: configs[1] (REC) and configs[3] (REC+RES), canvas 640 x 640.

Variants, alternated in ONE process on one model per configuration, a host clock around the call + a final synchronise, after one
warm-up call of each; every call includes its own capture, as a validation pass after an epoch does:
  raw       evaluate_raw(model, criterion, post, loader, device, canvas): per batch rt_raw_stage, rt_eval_raw_facts, one replay
            (REC+RES: rt_eval_orig inside the graph, the seven '_orig' keys on top);
  pipeline  the same items through DeviceInputPipeline(size, max_size, pad_to=canvas) where the collate would run it (the 18-launch
            chain, `size` / `orig_size` collated as tensors), then evaluate(canvas=canvas).

`--kernel` times rt_eval_orig alone on a B = 8 batch of 427 x 640 originals (logits 160 x 160, canvas 640 x 640) with the grid the
evaluation step gives it (max_pixels = 16 * 640 * 640: 400 chunks per image, of which an image fills 17) and with a grid cut to the
batch (max_pixels = 427 * 640), beside rt_eval_canvas on the same batch: 50 calls recorded into one hipGraph after a warm-up, one HIP
event pair around a replay, median of 5.

    python benchmarks/raw_eval.py [--batches 60] [--runs 5] [--variants raw,pipeline] [--shapes rec,res] [--kernel] [--out FILE]
"""
import argparse
import contextlib
import gc
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=60)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--variants", default="raw,pipeline")
ap.add_argument("--shapes", default="rec,res")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--out", default=None, help="append the result lines to this file")
a = ap.parse_args()

sys.path.insert(0, ROOT)
import bench                                     # noqa: E402  (synth_batch; puts the repository root on sys.path)
import torch                                     # noqa: E402
from reftr_amd import hip                        # noqa: E402
from reftr_amd.data import DeviceInputPipeline, RawImages          # noqa: E402
from reftr_amd.data.canvas import BatchCanvas    # noqa: E402
from reftr_amd.engine_vg import evaluate, evaluate_raw             # noqa: E402
from reftr_amd.models import layout as Lm        # noqa: E402
from reftr_amd.models.criterion import CriterionVGMultiPhrase, CriterionVGOnePhraseSeg       # noqa: E402
from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase         # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR                                         # noqa: E402

dev = torch.device("cuda")
B, S, L = 8, 640, 40
SHAPES = [(640, 640), (480, 640), (640, 480), (427, 640), (512, 640), (640, 427)]
out_lines = []


def say(line):
    print(line, flush=True)
    out_lines.append(line)


def raw_batch(h, w, seed, masks):
    """(samples with a RawImages, targets in the raw frame), pinned."""
    samples, targets = bench.synth_batch(B, h, w, L, "cpu", seed)
    g = torch.Generator().manual_seed(seed)
    s = {k: v.pin_memory() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = RawImages([torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(B)], min(h, w), S)
    assert s["img"].out_sizes() == [(h, w)] * B
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    tg = []
    for i, t in enumerate(targets):
        cx, cy, bw, bh = [float(v) for v in t["boxes"][0]]
        d = {"boxes": torch.tensor([[(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h]]),
             "labels": t["labels"], "image_id": torch.tensor(1000 * seed + i)}
        if masks:
            d["masks"] = ((((xx + 0.5) / w - cx).abs() < bw / 2) & (((yy + 0.5) / h - cy).abs() < bh / 2))[None].to(torch.uint8)
        tg.append({k: v.pin_memory() for k, v in d.items()})
    return s, tg


class Collated:
    """The loader of the `pipeline` variant: every raw item goes through DeviceInputPipeline(pad_to=canvas) as the collate would run
    it, and `orig_size` is collated as a tensor beside the pipeline's `size`."""

    def __init__(self, batches, pipes):
        self.batches, self.pipes = batches, pipes

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for s, t in self.batches:
            img = s["img"]
            key = (img.size, img.max_size)
            if key not in self.pipes:
                self.pipes[key] = DeviceInputPipeline(img.size, img.max_size, device="cuda", pad_to=(S, S))
            # (the targets cross first: the chain's target transforms -- the mask's `nearest` resize among them -- run on the device)
            t = [dict({k: v.to("cuda", non_blocking=True) for k, v in x.items()}, orig_size=torch.tensor([int(im.shape[0]), int(im.shape[1])]))
                 for x, im in zip(t, img.images)]
            nested, nt = self.pipes[key](img.images, t)
            yield dict(s, img=nested), nt


def loader_of(kinds, n, seed=7):
    g = torch.Generator().manual_seed(seed)
    order = []
    while len(order) < n:
        order += torch.randperm(len(kinds), generator=g).tolist()
    return [kinds[i] for i in order[:n]]


def make(masks):
    if masks:
        model = RefTR(Lm.ModelConfig(masks=True), device=dev, aux_loss=False)
        wd = {"loss_giou": 1.0, "loss_bbox": 1.0, "loss_dice": 1.0, "loss_mask": 1.0, "loss_cem": 1.0}
        crit = CriterionVGOnePhraseSeg(wd, ["masks", "boxes"])
        post = {"bbox": PostProcessVGMultiPhrase(), "segm": PostProcessSegm()}
    else:
        model = RefTR(Lm.ModelConfig(), device=dev, aux_loss=True)
        wd = {"loss_giou": 1.0, "loss_bbox": 1.0}
        wd.update({f"{k}_{i}": v for i in range(5) for k, v in list(wd.items())})
        crit = CriterionVGMultiPhrase(wd, ["boxes"])
        post = {"bbox": PostProcessVGMultiPhrase()}
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02); model.mark_dirty()
    return model, crit, post


def timed(fn, n):
    gc.collect()                 # the previous variant's captures go now, not inside this variant's first capture
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        stats, _ = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, stats


def kernel_time(n=50):
    g = torch.Generator().manual_seed(3)
    P, K, Q, h, w, oh, ow = 1, 1, 1, S // 4, S // 4, 427, 640
    cv = BatchCanvas(S, S, 1, masks=True)
    s, t = raw_batch(oh, ow, 5, True)
    s = {"img": s["img"].to("cuda"), "sentence": s["sentence"].cuda()}
    t = [{k: v.cuda() for k, v in tg.items()} for tg in t]
    st = cv.stage(s, t)
    boxes = torch.rand(B, P, K, 4, generator=g).cuda(); valid = torch.ones(B, P, K, dtype=torch.uint8, device="cuda")
    pm = torch.randn(B, Q, h, w, generator=g).cuda()
    facts = torch.zeros(B, 6, dtype=torch.int32, device="cuda"); ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    state = hip.EvalCanvasState(1 << 10, B, P, "cuda")
    masks = [x["masks"] for x in t]

    def orig(max_pixels):
        so = hip.EvalOrigState(B, max_pixels, "cuda")
        hip.eval_raw_facts([(oh, ow)] * B, [(oh, ow)] * B, (S, S), facts, ids, mask_list=masks, mask_table=so.mask_table, max_pixels=max_pixels)
        return lambda: hip.eval_orig(pm, facts, so, (S, S))

    def canvas():
        hip.eval_canvas(boxes, valid, st.targets_static[0], st.targets_static[1], facts, ids, state, pred_masks=pm, tgt_masks=st.tgt_masks)

    def us(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(n):
                fn()
        gr.replay(); torch.cuda.synchronize()
        res = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); gr.replay(); e1.record(); e1.synchronize()
            res.append(e0.elapsed_time(e1) / n * 1e3)
        return statistics.median(res), min(res), max(res)
    full = hip.RAW_STAGE_MAX_SCALE ** 2 * S * S
    for name, fn in ((f"rt_eval_orig, grid for max_pixels = 16 * {S} * {S} ({hip.eval_orig_chunks(full)} chunks per image)", orig(full)),
                     (f"rt_eval_orig, grid for max_pixels = {oh} * {ow} ({hip.eval_orig_chunks(oh * ow)} chunks per image)", orig(oh * ow)),
                     ("rt_eval_canvas (canvas frame 640x640)", canvas)):
        m, lo, hi = us(fn)
        say(f"kernel B={B} original {oh}x{ow} logits {h}x{w}: {name}: {m:.1f} us per call (min {lo:.1f} max {hi:.1f}; {n} calls in one graph, 5 replays)")


variants = [v for v in a.variants.split(",") if v]
for name, masks in (("REC configs[1]", False), ("REC+RES configs[3]", True)):
    if ("res" if masks else "rec") not in a.shapes.split(",") or not variants:
        continue
    model, crit, post = make(masks)
    canvas = BatchCanvas(S, S, 1, masks=masks)
    raw = loader_of([raw_batch(h, w, 1234 + i, masks) for i, (h, w) in enumerate(SHAPES)], a.batches)
    pipes = {}
    run = {"raw": lambda: evaluate_raw(model, crit, post, raw, dev, canvas),
           "pipeline": lambda: evaluate(model, crit, post, Collated(raw, pipes), dev, canvas=canvas)}
    ms, last = {v: [] for v in variants}, {}
    for r in range(a.runs + 1):                  # run 0 warms up every variant
        for v in variants:
            t, last[v] = timed(run[v], len(raw))
            if r:
                ms[v].append(t)
    for v in variants:
        say("%-20s %-10s %7.3f ms/batch (median of %d runs of %d batches of %d; min %.3f max %.3f)" % (
            name, v, statistics.median(ms[v]), a.runs, a.batches, B, min(ms[v]), max(ms[v])))
    if "raw" in ms and "pipeline" in ms:
        shared = [k for k in last["pipeline"] if last["raw"][k] == last["pipeline"][k] or last["raw"][k] != last["raw"][k]]
        say(f"{name}: {len(shared)} of {len(last['pipeline'])} keys of the pipeline variant equal in the raw variant; "
            + ", ".join(f"{k} = {last['raw'][k]:.4f}" for k in sorted(last["raw"]) if k.endswith("_orig")))
        say(f"{name}: slowest raw run {max(ms['raw']):.3f} ms vs fastest pipeline run {min(ms['pipeline']):.3f} ms -> "
            + ("raw faster in every run" if max(ms["raw"]) < min(ms["pipeline"]) else "NOT separated"))
    del model, crit, post, raw
    torch.cuda.empty_cache()
if a.kernel:
    kernel_time()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(out_lines) + "\n")
