"""reftr_amd.Predictor end to end -- raw images and phrases in, boxes and original-size masks on the host -- beside the composition
a user has to assemble by hand from the public pieces.

Shapes: configs[1] (REC: ResNet-50, B = 8, L = 40) and configs[3] (REC+RES: the same with the segmentation head); every batch holds
B = 8 raw 375 x 500 uint8 images in pinned host memory, resized to 480 x 640 (size 480, max_size 640) on a 640 x 640 canvas.

Variants, alternated in ONE process on one model per shape, a host clock around a run of `--batches` batches (each batch's results
are on the host when its call returns) after one warm-up run of each:
  predictor    Predictor(model, post, BatchCanvas(640, 640, 1), max_orig_size=(375, 500)): rt_raw_stage, rt_predict_facts, one replay,
               one copy, one wait per batch;
  composition  DeviceInputPipeline (the chain of profiles/raw_stage.txt) -> CapturedForward -> PostProcessVGMultiPhrase scaled to the
               original size -> PostProcessSegm (REC+RES) -> one .cpu() per image and result.  Every batch here has ONE shape, so the
               forward is one capture at the batch's own 480 x 640 -- three quarters of the canvas's pixels.

`--kernel` times rt_predict_canvas beside rt_box_postprocess + rt_mask_postprocess (with masks_origin) on the REC+RES batch's
tensors: 50 calls recorded into one hipGraph after a warm-up, one HIP event pair around a replay, median of 5.

    python benchmarks/predict_throughput.py [--batches 60] [--runs 5] [--shapes rec,res] [--kernel] [--out FILE]
"""
import argparse
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=60)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--shapes", default="rec,res")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--out", default=None, help="append the result lines to this file")
a = ap.parse_args()

sys.path.insert(0, ROOT)
import bench                                     # noqa: E402  (synth_batch)
import torch                                     # noqa: E402
from reftr_amd import Predictor, hip             # noqa: E402
from reftr_amd.data import RawImages             # noqa: E402
from reftr_amd.data.canvas import BatchCanvas    # noqa: E402
from reftr_amd.data.device_input import DeviceInputPipeline                                  # noqa: E402
from reftr_amd.engine_vg import CapturedForward  # noqa: E402
from reftr_amd.models import layout as Lm        # noqa: E402
from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase         # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR                                         # noqa: E402

dev = torch.device("cuda")
B, S, L, RAW_HW, SIZE, MAX_SIZE = 8, 640, 40, (375, 500), 480, 640
out_lines = []


def say(line):
    print(line, flush=True)
    out_lines.append(line)


def batch(seed):
    """One loader batch: B raw images and the token fields, pinned."""
    samples, _ = bench.synth_batch(B, 32, 32, L, "cpu", seed)
    g = torch.Generator().manual_seed(seed)
    s = {k: v.pin_memory() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = RawImages([torch.randint(0, 256, (*RAW_HW, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(B)], SIZE, MAX_SIZE)
    return s


def make(masks):
    model = RefTR(Lm.ModelConfig(masks=True), device=dev, aux_loss=False) if masks else RefTR(Lm.ModelConfig(), device=dev, aux_loss=True)
    post = {"bbox": PostProcessVGMultiPhrase(), "segm": PostProcessSegm()} if masks else {"bbox": PostProcessVGMultiPhrase()}
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02); model.mark_dirty()
    model.eval()
    return model, post


class Composition:
    """What a user assembles today: every stage waits on the host."""

    def __init__(self, model, post):
        self.pipe, self.fwd, self.post = DeviceInputPipeline(SIZE, MAX_SIZE, device=dev), CapturedForward(model), post

    @torch.no_grad()
    def __call__(self, s):
        img = s["img"]
        nested, tg = self.pipe(img.images, [{} for _ in img.images])
        on = {k: v.to(dev, non_blocking=True) for k, v in s.items() if k != "img"}
        on["img"] = nested
        out = self.fwd(on)
        orig = torch.tensor([[int(im.shape[0]), int(im.shape[1])] for im in img.images])
        results = self.post["bbox"](out, orig, scale_to_original_shape=True)
        res = [{"boxes": r["boxes"].cpu()} for r in results]
        if "segm" in self.post:
            sizes = torch.stack([t["size"] for t in tg])
            for r, m in zip(res, self.post["segm"]([{} for _ in tg], out, orig, sizes)):
                r["masks"] = m["masks_origin"].cpu()
        return res


def timed(fn, loader):
    gc.collect()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for s in loader:
        fn(s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(loader)


def kernel_time(n=50):
    g = torch.Generator().manual_seed(3)
    P, K, Q, h, w = 1, 1, 1, S // 4, S // 4
    sizes, origs = [(480, 640)] * B, [RAW_HW] * B
    boxes = torch.rand(B, P, K, 4, generator=g).cuda(); valid = torch.ones(B, P, K, dtype=torch.uint8, device="cuda")
    pm = torch.randn(B, Q, h, w, generator=g).cuda()
    st = hip.PredictState(B, P, "cuda", mask_capacity=B * 16 * -(-(Q * RAW_HW[0] * RAW_HW[1]) // 16))
    hip.predict_facts(sizes, origs, (S, S), st.facts, Q=Q, capacity=st.capacity)
    sizes_i32, orig_i32 = torch.tensor(sizes, dtype=torch.int32).cuda(), torch.tensor(origs, dtype=torch.int32).cuda()
    orig_f = torch.tensor(origs, dtype=torch.float32).cuda()
    n_px = Q * RAW_HW[0] * RAW_HW[1]
    off = torch.arange(B + 1, dtype=torch.int64).cuda() * n_px

    def new():
        hip.predict_canvas(boxes, valid, st, pred_masks=pm, canvas_hw=(S, S))

    def old(frame_hw):
        def fn():
            hip.mask_postprocess(pm, sizes_i32, frame_hw, orig_i32=orig_i32, origin_off=off, origin_total=B * n_px, max_origin=RAW_HW[0] * RAW_HW[1])
            hip.box_postprocess(boxes, valid, orig_f)
        return fn

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
    rows = {}
    for key, name, fn in (("new", "rt_predict_canvas (boxes + masks_origin, no frame)", new),
                          ("old", "rt_box_postprocess + rt_mask_postprocess, frame 480x640 (today's frame)", old((480, 640))),
                          ("old_cv", "rt_box_postprocess + rt_mask_postprocess, frame 640x640 (the canvas as frame)", old((S, S)))):
        rows[key] = us(fn)
        m, lo, hi = rows[key]
        say(f"kernel B={B} raw 375x500 resized 480x640 logits {h}x{w}: {name}: {m:.1f} us per call (min {lo:.1f} max {hi:.1f}; {n} calls in one graph, 5 replays)")
    say("kernel: slowest rt_predict_canvas replay %.1f us vs fastest replay of the two launches (today's frame) %.1f us -> %s" % (
        rows["new"][2], rows["old"][1], "the kernel alone is faster in every replay" if rows["new"][2] < rows["old"][1]
        else "the kernel alone is NOT faster than the two it replaces"))


for name, masks in (("REC configs[1]", False), ("REC+RES configs[3]", True)):
    if ("res" if masks else "rec") not in a.shapes.split(","):
        continue
    model, post = make(masks)
    loader = [batch(1234 + i) for i in range(6)] * (-(-a.batches // 6))
    loader = loader[:a.batches]
    variants = {"predictor": Predictor(model, post, BatchCanvas(S, S, 1), max_orig_size=RAW_HW), "composition": Composition(model, post)}
    got, want = variants["predictor"](loader[0]), variants["composition"](loader[0])
    say(f"{name}: result structure of both variants: " + ", ".join(f"{k} {tuple(v.shape)} {str(v.dtype).split('.')[-1]}" for k, v in got[0].items())
        + ("" if all(sorted(x) == sorted(y) and all(x[k].shape == y[k].shape for k in x) for x, y in zip(got, want)) else "  (DIFFER)"))
    ms = {v: [] for v in variants}
    for r in range(a.runs + 1):                  # run 0 warms up every variant
        for v, fn in variants.items():
            t = timed(fn, loader)
            if r:
                ms[v].append(t)
    for v in variants:
        say("%-20s %-12s %7.3f ms/batch (median of %d runs of %d batches of %d; min %.3f max %.3f)" % (
            name, v, statistics.median(ms[v]), a.runs, a.batches, B, min(ms[v]), max(ms[v])))
    say(f"{name}: slowest predictor run {max(ms['predictor']):.3f} ms vs fastest composition run {min(ms['composition']):.3f} ms -> "
        + ("predictor faster in every run" if max(ms["predictor"]) < min(ms["composition"]) else "NOT separated"))
    del model, post, loader, variants
    torch.cuda.empty_cache()
if a.kernel:
    kernel_time()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(out_lines) + "\n")
