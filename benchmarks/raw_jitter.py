"""The colour jitter of raw training batches on the device (rt_hsv_jitter, RawImages.gains): what it costs.

Four measurements:

  (a) kernel   rt_hsv_jitter alone: B = 8 raw 375 x 500 images into a scratch at 16-byte aligned offsets (as BatchCanvas stages them),
               `--calls` calls recorded into one hipGraph after warm-up, one event pair around a replay, median of `--runs` with
               min - max -- like the neighbouring kernel figures (benchmarks/raw_stage.py).  This figure is also the MOST that fusing
               the jitter into rt_raw_stage's horizontal pass could save per batch.
  (b) epoch    train_one_epoch(canvas=) over benchmarks/ragged_epoch.py's cfg1 workload as RAW host batches (R50, B = 8, L = 40, one box
               per image; six raw shapes that resize at size = max_size = 640 to cfg1's six: 500 x 500 -> 640 x 640, 375 x 500 ->
               480 x 640, 500 x 375, 333 x 500 -> 426 x 640, 400 x 500 -> 512 x 640, 500 x 333), the same batches WITHOUT and WITH
               gains, alternated run by run on one model and one capture; median of `--runs` epochs of `--batches` batches, min - max.
  (c) host     reftr_amd.data.jitter.apply on the same eight 375 x 500 images on the CPU: the package's plain-torch DEFINITION of the
               jitter, NOT cv2 (which is not installed here): it says what the definition costs, and no claim against cv2 follows.
  (d) parent   with `--baseline-root DIR` (a checkout of the parent commit with its library built): the un-jittered raw epoch of (b) in
               child processes, the parent's package and this one alternated, two each, before this process touches the GPU.  The
               no-gains path is today's path: its figure has to lie within the parent's run-to-run spread.

    python benchmarks/raw_jitter.py [--runs 5] [--batches 60] [--calls 50] [--baseline-root DIR] [--out FILE]

The jittered figures are reported, not gated."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--batches", type=int, default=60)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--out", default=None, help="append the result lines to this file")
ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()

RAW_SHAPES = [(500, 500), (375, 500), (500, 375), (333, 500), (400, 500), (500, 333)]
SIZE = 640


def child_epochs(root):
    """The un-jittered raw epoch in a fresh process against the package under `root` -> ms per iteration of each run."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--batches", str(a.batches), "--batch", str(a.batch),
                          "--package-root", os.path.abspath(root), "--child"], check=True, timeout=900, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


parent_ms, this_ms = [], []
if a.baseline_root and not a.child:          # fresh children, alternated, before this process touches the GPU
    for _ in range(2):
        parent_ms += child_epochs(a.baseline_root)
        this_ms += child_epochs(ROOT)

sys.path.insert(0, ROOT)
import bench                                               # noqa: E402  (synth_batch; puts the repository root on sys.path)
sys.path.insert(0, a.package_root)                         # ... in front of which the package under test goes
import torch                                               # noqa: E402
from reftr_amd.data import RawImages                       # noqa: E402
from reftr_amd.data.canvas import BatchCanvas              # noqa: E402
from reftr_amd.engine_vg import train_one_epoch            # noqa: E402
from reftr_amd.models import layout as Lm                  # noqa: E402
from reftr_amd.models.criterion import CriterionVGMultiPhrase  # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR       # noqa: E402
from reftr_amd.optim import FusedAdamW                     # noqa: E402


def spread(xs, unit="us", fmt=".1f"):
    return f"{statistics.median(xs):{fmt}} {unit} (min {min(xs):{fmt}} - max {max(xs):{fmt}})"


def raw_kinds(B, gains):
    """cfg1's six batch kinds as pinned raw host batches: token fields and one box per image from bench.synth_batch, boxes as xyxy
    pixels of the raw frame; `gains`: every image carries a (1, v_gain) drawn once from a seeded generator."""
    import random
    rng = random.Random(99)
    kinds = []
    for i, (h, w) in enumerate(RAW_SHAPES):
        s, t = bench.synth_batch(B, 32, 32, 40, "cpu", 1234 + i)
        g = torch.Generator().manual_seed(1234 + i)
        imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(B)]
        kw = {"gains": [(1.0, (rng.random() * 2 - 1) * 0.5 + 1) for _ in range(B)]} if gains else {}
        samples = {k: v.pin_memory() for k, v in s.items() if k not in ("img", "img_mask")}
        samples["img"] = RawImages(imgs, SIZE, SIZE, **kw)
        targets = []
        for tg in t:
            cx, cy, bw, bh = tg["boxes"].unbind(-1)
            xyxy = torch.stack([(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h], dim=-1)
            targets.append({"boxes": xyxy.pin_memory(), "labels": tg["labels"].pin_memory()})
        kinds.append((samples, targets))
    return kinds


class Loader:
    def __init__(self, n, kinds, seed):
        g = torch.Generator().manual_seed(seed)
        self.n, self.kinds, self.order = n, kinds, []
        while len(self.order) < n:
            self.order += torch.randperm(len(kinds), generator=g).tolist()

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.kinds[self.order[i]]


def build():
    cfg = Lm.ModelConfig()
    model = RefTR(cfg, device=torch.device("cuda"), aux_loss=True)
    wd = {"loss_giou": 1.0, "loss_bbox": 1.0}
    wd.update({f"{k}_{i}": v for i in range(cfg.dec_layers - 1) for k, v in list(wd.items())})
    crit = CriterionVGMultiPhrase(wd, ["boxes"])
    torch.manual_seed(1234)
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02)
    model.mark_dirty()
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    return model, crit, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=100000)


def epochs(variants):
    """{name: [ms per iteration of each run]} of train_one_epoch(canvas=) over the loaders of `variants` ({name: kinds}), alternated run
    by run on one model and one canvas, after a warm-up epoch of each; also the number of captures."""
    model, crit, opt, sched = build()
    cv = BatchCanvas(SIZE, SIZE, 1)
    ms = {name: [] for name in variants}
    with contextlib.redirect_stdout(io.StringIO()):        # the loop's progress lines
        for kinds in variants.values():
            train_one_epoch(model, crit, Loader(2 * len(kinds), kinds, 7), opt, sched, torch.device("cuda"), 0, max_norm=0.1, canvas=cv)
        torch.cuda.synchronize()
        for r in range(a.runs):
            for name, kinds in variants.items():
                loader = Loader(a.batches, kinds, 11 + r)
                t0 = time.perf_counter()
                train_one_epoch(model, crit, loader, opt, sched, torch.device("cuda"), 1 + r, max_norm=0.1, canvas=cv)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / a.batches * 1e3)
    return ms, len(model._captured_steps)


def kernel_us():
    """(a): rt_hsv_jitter alone, and the bytes it moves."""
    from reftr_amd import hip as H
    B, (h, w), n = a.batch, (375, 500), a.calls
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(B)]
    gains = [(1.0, 0.5 + b / B) for b in range(B)]
    step = -(-h * w * 3 // 16) * 16
    scratch = torch.empty(B * step, dtype=torch.uint8, device="cuda")
    outs = [scratch[b * step:b * step + h * w * 3].view(h, w, 3) for b in range(B)]
    fn = lambda: H.hsv_jitter(imgs, gains, outs)           # noqa: E731
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            fn()
    graph.replay(); torch.cuda.synchronize()
    us = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); graph.replay(); e1.record(); e1.synchronize()
        us.append(e0.elapsed_time(e1) / n * 1e3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        fn()
    host = (time.perf_counter() - t0) / 200 * 1e6          # issue cost on the host (the queue never fills at this count)
    torch.cuda.synchronize()
    return us, host, 2 * B * h * w * 3, [im.cpu() for im in imgs], gains, [o.cpu() for o in outs]


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if a.child:
        ms, _ = epochs({"plain": raw_kinds(a.batch, False)})
        print(json.dumps(ms["plain"]))
        return
    from reftr_amd.data import jitter
    B = a.batch
    us, host_us, moved, imgs, gains, outs = kernel_us()
    host_ms = []
    for r in range(a.runs):                                # (c) the definition on the CPU, the same eight images
        t0 = time.perf_counter()
        want = [jitter.apply(im, *g) for im, g in zip(imgs, gains)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert all(torch.equal(o, w) for o, w in zip(outs, want)), "rt_hsv_jitter and jitter.apply disagree"
    ms, captures = epochs({"plain": raw_kinds(B, False), "jittered": raw_kinds(B, True)})
    med = statistics.median
    lines = [
        f"raw_jitter B={B}, {a.runs} runs",
        f"  (a) rt_hsv_jitter alone, B={B} 375x500, {a.calls} calls in one graph, launch to idle: {spread(us)} per call; {moved / 1e6:.1f} MB moved "
        f"(read + written), {moved / med(us) / 1e6:.2f} TB/s; hip.hsv_jitter costs the host {host_us:.0f} us per call; output bytes equal "
        f"jitter.apply's.  Fusing it into rt_raw_stage could save at most this {med(us):.1f} us per batch.",
        f"  (b) raw cfg1 epoch, train_one_epoch(canvas=), {a.batches} batches per run, alternated, {captures} capture(s):",
        f"        without gains {spread(ms['plain'], 'ms/iteration', '.3f')}",
        f"        with gains    {spread(ms['jittered'], 'ms/iteration', '.3f')}   (median difference "
        f"{(med(ms['jittered']) - med(ms['plain'])) * 1e3:+.1f} us per batch; reported, not gated)",
        f"  (c) jitter.apply on the CPU, the same {B} images (the plain-torch definition, NOT cv2; {torch.get_num_threads()} torch threads): "
        f"{spread(host_ms, 'ms', '.1f')} per batch",
    ]
    if parent_ms:
        lo, hi = min(parent_ms), max(parent_ms)
        inside = lo <= med(this_ms) <= hi
        lines += [
            f"  (d) un-jittered raw epoch in child processes, parent and this alternated (2 x {a.runs} runs each):",
            f"        parent {spread(parent_ms, 'ms/iteration', '.3f')}",
            f"        this   {spread(this_ms, 'ms/iteration', '.3f')}   -> median "
            + ("within the parent's run-to-run spread" if inside else f"OUTSIDE the parent's spread by {min(abs(med(this_ms) - lo), abs(med(this_ms) - hi)) * 1e3:.1f} us"),
        ]
    for line in lines:
        print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
