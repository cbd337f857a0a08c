"""engine_vg.evaluate() end to end over a validation loader whose batches all differ in shape, with and without the batch canvas.

Shapes: configs[1] (REC: ResNet-50, B = 8, L = 40, aux losses) and configs[3] (REC+RES: the same with the segmentation head and a
target mask per image); the image shape of a batch is one of {640x640, 480x640, 640x480, 427x640, 512x640, 640x427} (the reference's
collate pads a batch to ITS largest image), a seeded shuffle of every block of six.  Batches are seeded and pinned.

Variants, alternated in ONE process on one model per shape, a host clock around evaluate() + a final synchronise, after one warm-up
call of each; every call includes its own captures, as a validation pass after an epoch does:
  canvas    evaluate(..., canvas=BatchCanvas(640, 640, 1)): one capture, every batch staged and replayed;
  nocanvas  the same loader without a canvas: four forward shapes captured, the others eager, the per-batch tail at its own shape;
  fixed     every batch 640 x 640, no canvas (the loop the canvas is not on).
`--baseline-root DIR` first runs nocanvas and fixed in a child process against the package checked out (and built) under DIR -- the
parent commit -- reported as 'parent nocanvas' / 'parent fixed'.

`--kernel` times rt_eval_canvas beside the three launches it replaces (rt_box_postprocess + rt_mask_postprocess + rt_eval_metrics; the
table's host-to-device copy is not in it) on a 640 x 640 REC+RES batch: 50 calls recorded into one hipGraph after a warm-up, one HIP
event pair around a replay, median of 5.

    python benchmarks/ragged_eval.py [--batches 60] [--runs 5] [--variants canvas,nocanvas,fixed] [--baseline-root DIR] [--kernel]
"""
import argparse
import contextlib
import gc
import io
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=60)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--variants", default="canvas,nocanvas,fixed")
ap.add_argument("--shapes", default="rec,res")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--out", default=None, help="append the result lines to this file")
ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
ap.add_argument("--tag", default="", help=argparse.SUPPRESS)
a = ap.parse_args()

if a.baseline_root:          # a fresh child, before this process touches the GPU
    cmd = [sys.executable, os.path.abspath(__file__), "--batches", str(a.batches), "--runs", str(a.runs), "--variants", "nocanvas,fixed",
           "--shapes", a.shapes, "--package-root", os.path.abspath(a.baseline_root), "--tag", "parent "]
    subprocess.run(cmd + (["--out", a.out] if a.out else []), check=True, timeout=900)

sys.path.insert(0, ROOT)
import bench                                     # noqa: E402  (synth_batch; puts the repository root on sys.path)
sys.path.insert(0, a.package_root)               # ... in front of which the package under test goes
import torch                                     # noqa: E402
from reftr_amd.engine_vg import evaluate         # noqa: E402
from reftr_amd.models import layout as Lm        # noqa: E402
from reftr_amd.models.criterion import CriterionVGMultiPhrase, CriterionVGOnePhraseSeg       # noqa: E402
from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase         # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR                                         # noqa: E402
from reftr_amd.util.misc import NestedTensor     # noqa: E402

dev = torch.device("cuda")
B, S, L = 8, 640, 40
SHAPES = [(640, 640), (480, 640), (640, 480), (427, 640), (512, 640), (640, 427)]
out_lines = []


def say(line):
    print(line, flush=True)
    out_lines.append(line)


def batch(h, w, seed, masks):
    samples, targets = bench.synth_batch(B, h, w, L, "cpu", seed)
    s = {k: v.pin_memory() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].pin_memory(), samples["img_mask"].pin_memory())
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    tg = []
    for i, t in enumerate(targets):
        d = dict(t, size=torch.tensor([h, w]), orig_size=torch.tensor([h, w]), image_id=torch.tensor(1000 * seed + i))
        if masks:
            cx, cy, bw, bh = [float(v) for v in t["boxes"][0]]
            d["masks"] = ((((xx + 0.5) / w - cx).abs() < bw / 2) & (((yy + 0.5) / h - cy).abs() < bh / 2))[None]
        tg.append({k: v.pin_memory() for k, v in d.items()})
    return s, tg


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


def timed(model, crit, post, loader, canvas):
    kw = {"canvas": canvas} if canvas is not None else {}
    gc.collect()                 # the previous variant's captures go now, not inside this variant's first capture
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        stats, _ = evaluate(model, crit, post, loader, dev, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(loader), stats


def kernel_time(n=50):
    from reftr_amd import hip
    from reftr_amd.data.canvas import BatchCanvas
    from reftr_amd.metrics import build_table
    g = torch.Generator().manual_seed(3)
    P, K, Q, h, w = 1, 1, 1, S // 4, S // 4
    cv = BatchCanvas(S, S, 1, masks=True)
    s, t = batch(427, 640, 5, True)
    s = {"img": NestedTensor(s["img"].tensors.cuda(), s["img"].mask.cuda()), "sentence": s["sentence"].cuda()}
    t = [{k: v.cuda() for k, v in tg.items()} for tg in t]
    st = cv.stage(s, t)
    boxes = torch.rand(B, P, K, 4, generator=g).cuda(); valid = torch.ones(B, P, K, dtype=torch.uint8, device="cuda")
    pm = torch.randn(B, Q, h, w, generator=g).cuda()
    facts = torch.zeros(B, 6, dtype=torch.int32, device="cuda"); ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    hip.eval_facts([x["size"] for x in t], facts, ids, origs=[x["orig_size"] for x in t], ids=[x["image_id"] for x in t],
                   mask_hw=[x["masks"].shape[-2:] for x in t])
    state = hip.EvalCanvasState(1 << 10, B, P, "cuda")
    sizes = [[427, 640]] * B
    words, keep = build_table(t, sizes)
    table = words.cuda()
    sizes_i32 = torch.tensor(sizes, dtype=torch.int32).cuda(); orig_f = torch.tensor(sizes, dtype=torch.float32).cuda()
    acc = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")

    def new():
        hip.eval_canvas(boxes, valid, st.targets_static[0], st.targets_static[1], facts, ids, state, pred_masks=pm, tgt_masks=st.tgt_masks)

    def old(frame_hw):
        def fn():
            frame, _ = hip.mask_postprocess(pm, sizes_i32, frame_hw)
            hip.box_postprocess(boxes, valid, orig_f)
            hip.eval_metrics(boxes, valid, table[:5 * B].view(B, 5), acc, masks=frame, sizes_i32=table[5 * B:].view(torch.int32).view(B, 2))
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
    for name, fn in (("rt_eval_canvas (canvas frame 640x640)", new), ("the three launches, frame 427x640 (today's frame)", old((427, 640))),
                     ("the three launches, frame 640x640 (the canvas as frame)", old((S, S)))):
        m, lo, hi = us(fn)
        say(f"kernel B={B} image 427x640 logits {h}x{w}: {name}: {m:.1f} us per call (min {lo:.1f} max {hi:.1f}; {n} calls in one graph, 5 replays)")


variants = [v for v in a.variants.split(",") if v]
for name, masks in (("REC configs[1]", False), ("REC+RES configs[3]", True)):
    if ("res" if masks else "rec") not in a.shapes.split(",") or not variants:
        continue
    model, crit, post = make(masks)
    ragged = loader_of([batch(h, w, 1234 + i, masks) for i, (h, w) in enumerate(SHAPES)], a.batches)
    fixed = loader_of([batch(S, S, 1300 + i, masks) for i in range(2)], a.batches)
    canvas = None
    if "canvas" in variants:
        from reftr_amd.data.canvas import BatchCanvas
        canvas = BatchCanvas(S, S, 1, masks=masks)
    ms = {v: [] for v in variants}
    for r in range(a.runs + 1):                  # run 0 warms up every variant
        for v in variants:
            t, stats = timed(model, crit, post, fixed if v == "fixed" else ragged, canvas if v == "canvas" else None)
            if r:
                ms[v].append(t)
    for v in variants:
        say("%-20s %-16s %7.3f ms/batch (median of %d runs of %d batches of %d; min %.3f max %.3f)" % (
            name, a.tag + v, statistics.median(ms[v]), a.runs, a.batches, B, min(ms[v]), max(ms[v])))
    if "canvas" in ms and "nocanvas" in ms:
        say(f"{name}: slowest canvas run {max(ms['canvas']):.3f} ms vs fastest no-canvas run {min(ms['nocanvas']):.3f} ms -> "
            + ("canvas faster in every run" if max(ms["canvas"]) < min(ms["nocanvas"]) else "NOT separated"))
    del model, crit, post, ragged, fixed
    torch.cuda.empty_cache()
if a.kernel:
    kernel_time()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(out_lines) + "\n")
