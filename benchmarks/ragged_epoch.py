"""train_one_epoch over a loader whose batches all differ in shape -- what a real loader produces -- with and without the batch canvas.

Two workloads, each a seeded synthetic loader of pinned host batches (built like benchmarks/epoch_throughput.py's):

  cfg1  configs[1]: R50, B = 8, L = 40, one box per image; the image shape of a batch is drawn from {640x640, 480x640, 640x480,
        427x640, 512x640, 640x427} (util/collate_fn.py:24-41 pads a batch to ITS largest image); six shapes within any six batches.
  cfg5  configs[4]-like: R101, 800 x 800, L = 90, 16 phrase slots x 22 tokens, ragged box counts as in benchmarks/cfg5_stress.py,
        another count pattern in every batch (eight patterns).

Variants, each on a fresh model, timed by host clock around an epoch that ends in a device synchronise, after a warm-up epoch that
visits every shape:
  canvas    train_one_epoch(..., canvas=BatchCanvas): one capture, every batch staged by rt_batch_stage and replayed;
  nocanvas  the same loader without a canvas: the first four shapes are captured, the others run the eager step;
  fixed     the floor: every batch has the one full-size shape (cfg5: one count pattern), no canvas.
`--variants nocanvas,fixed` runs on a checkout without the canvas (the parent commit's figure).

`--kernel` times rt_batch_stage alone (50 launches recorded into one hipGraph after warm-up, one HIP event pair around a replay,
median of 5) beside torch's copy_ of the same image bytes, measured the same way in the same process.

    python benchmarks/ragged_epoch.py --workload cfg1 [--runs 5] [--batches 60] [--variants canvas,nocanvas,fixed] [--kernel]

Prints one line per variant: median and min-max ms per iteration over the runs, captures and eager steps."""
import argparse
import contextlib
import gc
import io
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from reftr_amd import engine_vg  # noqa: E402
from reftr_amd.engine_vg import train_one_epoch  # noqa: E402
from reftr_amd.models import layout as Lm  # noqa: E402
from reftr_amd.models.criterion import CriterionVGMultiPhrase  # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR  # noqa: E402
from reftr_amd.optim import FusedAdamW  # noqa: E402
from reftr_amd.util.misc import NestedTensor  # noqa: E402

CFG1_SHAPES = [(640, 640), (480, 640), (640, 480), (427, 640), (512, 640), (640, 427)]


def _pin(samples, targets):
    s = {k: v.pin_memory() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].pin_memory(), samples["img_mask"].pin_memory())
    return s, [{k: v.pin_memory() for k, v in tg.items()} for tg in targets]


def cfg5_batch(B, size, P, rot, seed):
    """benchmarks/cfg5_stress.py's batch; image b has max(1, P - 2 * ((b + rot) % B)) boxes / valid phrases."""
    L, Lp = 90, 22
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, size, size, generator=g); mask = torch.zeros(B, size, size, dtype=torch.bool)
    for b in range(1, B, 2):
        mask[b, :, (size * 3) // 4:] = True; img[b, :, :, (size * 3) // 4:] = 0
    ids = torch.zeros(B, L, dtype=torch.long); sm = torch.zeros(B, L, dtype=torch.long)
    ph = torch.zeros(B, P, Lp, dtype=torch.long); pm = torch.zeros(B, P, Lp, dtype=torch.long)
    pl = torch.zeros(B, P, dtype=torch.long); pr = torch.ones(B, P, dtype=torch.long)
    targets = []
    for b in range(B):
        n = int(torch.randint(40, L + 1, (1,), generator=g))
        ids[b, :n] = torch.randint(1000, 30000, (n,), generator=g); ids[b, 0] = 101; ids[b, n - 1] = 102; sm[b, :n] = 1
        nv = max(1, P - 2 * ((b + rot) % B))
        for j in range(P):
            if j < nv:
                k = 3 + (j % 5)
                ph[b, j, :k] = torch.randint(1000, 30000, (k,), generator=g); ph[b, j, 0] = 101; ph[b, j, k - 1] = 102; pm[b, j, :k] = 1
                pl[b, j] = 1 + 2 * j; pr[b, j] = 1 + 2 * j + (k - 2)
            else:
                ph[b, j, 0] = 101; ph[b, j, 1] = 102; pm[b, j, :2] = 1
        u = torch.rand(nv, 4, generator=g)
        targets.append({"boxes": torch.stack([0.3 + 0.4 * u[:, 0], 0.3 + 0.4 * u[:, 1], 0.1 + 0.4 * u[:, 2], 0.1 + 0.4 * u[:, 3]], -1),
                        "labels": torch.zeros(nv, dtype=torch.long)})
    samples = {"img": img, "img_mask": mask, "sentence": ids, "sentence_mask": sm, "phrase": ph, "phrase_mask": pm,
               "phrase_pos_l": pl, "phrase_pos_r": pr}
    return samples, targets


class RaggedLoader:
    """`n` batches per epoch; batch i is kinds[order[i % len]], the order a seeded shuffle of every block of len(kinds) batches, so
    that every kind appears once in any aligned block."""

    def __init__(self, n, kinds, seed=7):
        self.n, self.kinds = n, kinds
        g = torch.Generator().manual_seed(seed)
        self.order = []
        while len(self.order) < n:
            self.order += torch.randperm(len(kinds), generator=g).tolist()

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.kinds[self.order[i]]


def build(workload):
    dev = torch.device("cuda")
    cfg = Lm.ModelConfig() if workload == "cfg1" else Lm.ModelConfig(resnet_layers=(3, 4, 23, 3))
    model = RefTR(cfg, device=dev, aux_loss=True)
    wd = {"loss_giou": 1.0, "loss_bbox": 1.0}
    wd.update({f"{k}_{i}": v for i in range(cfg.dec_layers - 1) for k, v in list(wd.items())})
    crit = CriterionVGMultiPhrase(wd, ["boxes"])
    torch.manual_seed(1234)
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02)
    model.mark_dirty()
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    return model, crit, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=100000)


def kinds_of(workload, B):
    if workload == "cfg1":
        ragged = [_pin(*bench.synth_batch(B, h, w, 40, "cpu", 1234 + i)) for i, (h, w) in enumerate(CFG1_SHAPES)]
        fixed = [_pin(*bench.synth_batch(B, 640, 640, 40, "cpu", 1300 + i)) for i in range(2)]
        return ragged, fixed, (640, 640, 1)
    ragged = [_pin(*cfg5_batch(B, 800, 16, rot, 50 + rot)) for rot in range(8)]
    fixed = [_pin(*cfg5_batch(B, 800, 16, 0, 90 + i)) for i in range(2)]
    return ragged, fixed, (800, 800, 16)


def run_variant(workload, variant, kinds, canvas_spec, runs, batches, out):
    model, crit, opt, sched = build(workload)
    kw = {}
    if variant == "canvas":
        from reftr_amd.data.canvas import BatchCanvas
        kw["canvas"] = BatchCanvas(*canvas_spec)
    sink = io.StringIO()                              # the loop's progress lines
    with contextlib.redirect_stdout(sink):
        train_one_epoch(model, crit, RaggedLoader(3 * len(kinds), kinds), opt, sched, torch.device("cuda"), 0, max_norm=0.1, **kw)
        torch.cuda.synchronize()
        ms, loaders = [], []
        for r in range(runs):
            loader = RaggedLoader(batches, kinds, seed=11 + r)
            t0 = time.perf_counter()
            stats = train_one_epoch(model, crit, loader, opt, sched, torch.device("cuda"), 1 + r, max_norm=0.1, **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / batches * 1e3)
            loaders.append(loader)
    # a timed step ran eagerly iff no capture holds its key (the captures were all made in the warm-up epoch)
    held = {k[0] for k in model._captured_steps}
    cv = kw.get("canvas")

    def key_of(b):
        return cv.key(b[0]) if cv is not None and cv.fits(*b) else engine_vg.CapturedTrainStep.shape_key(*b)
    eager_timed = sum(key_of(b) not in held for loader in loaders for b in loader)
    shapes = len({engine_vg.CapturedTrainStep.shape_key(*b) for b in list(RaggedLoader(20, kinds, seed=11))})
    line = (f"{workload} {variant:9s}: median {statistics.median(ms):7.3f} ms/iteration (min {min(ms):.3f} - max {max(ms):.3f}, {runs} runs of "
            f"{batches} batches), {len(model._captured_steps)} capture(s), {eager_timed} of {runs * batches} timed steps eager, "
            f"{shapes} shapes in the first 20 batches, loss {stats.get('loss'):.4f}")
    print(line); out.append(line)
    return ms


def kernel_time(out, B=8, src=(427, 640), size=640, n=50):
    from reftr_amd.data.canvas import BatchCanvas
    cv = BatchCanvas(size, size, 1)
    s, t = bench.synth_batch(B, src[0], src[1], 40, "cpu", 5)
    s = {"img": NestedTensor(s["img"].cuda(), s["img_mask"].cuda()), "sentence": s["sentence"].cuda()}
    t = [{k: v.cuda() for k, v in tg.items()} for tg in t]
    dst = cv.stage(s, t)
    full = torch.randn(B, 3, size, size, device="cuda"); full_dst = torch.empty_like(full)
    same = torch.empty_like(s["img"].tensors)

    def timed(fn):
        """us per launch: `n` launches recorded into one hipGraph (the host's launch cost stays out), one event pair around a replay."""
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                fn()
        g.replay(); torch.cuda.synchronize()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); e1.synchronize()
            best.append(e0.elapsed_time(e1) / n * 1e3)
        return statistics.median(best)
    t_stage = timed(lambda: cv.stage(s, t, out=dst))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        cv.stage(s, t, out=dst)
    host_us = (time.perf_counter() - t0) / 200 * 1e6          # issue cost on the host (the queue never fills at this count)
    torch.cuda.synchronize()
    t_full = timed(lambda: full_dst.copy_(full))
    t_src = timed(lambda: same.copy_(s["img"].tensors))
    wr = B * 3 * size * size * 4 + B * size * size
    rd = B * 3 * src[0] * src[1] * 4 + B * src[0] * src[1]
    line = (f"rt_batch_stage B={B} {src[0]}x{src[1]} -> {size}x{size}: {t_stage:.1f} us per launch ({n} launches in one graph, median of 5 replays; "
            f"BatchCanvas.stage costs the host {host_us:.0f} us per call; {(wr + rd) / t_stage / 1e6:.2f} TB/s "
            f"of {wr / 1e6:.1f} MB written + {rd / 1e6:.1f} MB read); torch copy_ of the canvas image bytes ({B * 3 * size * size * 4 / 1e6:.1f} MB): "
            f"{t_full:.1f} us; of the source image bytes: {t_src:.1f} us")
    print(line); out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("cfg1", "cfg5"), default="cfg1")
    ap.add_argument("--variants", default="canvas,nocanvas,fixed")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = []
    variants = [x for x in a.variants.split(",") if x]
    ragged, fixed, spec = kinds_of(a.workload, a.batch) if variants else (None, None, None)
    res = {}
    for v in variants:
        res[v] = run_variant(a.workload, v, fixed if v == "fixed" else ragged, spec, a.runs, a.batches, out)
        gc.collect()                                     # the variant's model and captures go while the device is idle
        torch.cuda.synchronize(); torch.cuda.empty_cache()
    if "canvas" in res and "nocanvas" in res:
        line = (f"{a.workload}: slowest canvas run {max(res['canvas']):.3f} ms vs fastest no-canvas run {min(res['nocanvas']):.3f} ms -> "
                + ("canvas faster in every run" if max(res["canvas"]) < min(res["nocanvas"]) else "NOT separated"))
        print(line); out.append(line)
    if a.kernel:
        kernel_time(out)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
