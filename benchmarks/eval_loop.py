"""engine_vg.evaluate() itself, timed end to end: the loop around the forward (criterion, post-processors, metrics, results dict), which
benchmarks/eval_throughput.py leaves out.  configs[1]'s shapes (REC: ResNet-50, 640 x 640, batch 8, aux losses) and configs[3]'s (REC+RES:
the same with the segmentation head and 640 x 640 target masks), a loader of identical pinned batches.

Per shape, in ONE process, evaluate() runs with REFTR_EVAL_METRICS=1 (metrics.EvalMeter: two launches per batch) and =0 (the per-image
torch loop) alternately, `--rounds` times each after one warm-up run of each, a host clock around evaluate() + a final synchronise.
`--baseline-root DIR` first runs the same measurement in a child process against the package checked out under DIR (the parent
commit, built there): its evaluate() has no switch and is reported as 'baseline'.  Printed per variant: the median ms per batch over
the rounds and the spread (min .. max).  Every evaluate() call captures its forward graph anew; that cost is in all variants alike.

    python benchmarks/eval_loop.py [--batches 40] [--rounds 5] [--baseline-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
ap.add_argument("--as-baseline", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()

if a.baseline_root:          # a fresh child, before this process touches the GPU
    subprocess.run([sys.executable, os.path.abspath(__file__), "--batches", str(a.batches), "--rounds", str(a.rounds),
                    "--package-root", os.path.abspath(a.baseline_root), "--as-baseline"], check=True, timeout=600)

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


def pinned(t):
    return t.pin_memory() if torch.is_tensor(t) else t


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
    samples, targets = bench.synth_batch(B, S, S, L, "cpu", 1234)
    s = {k: pinned(v) for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(pinned(samples["img"]), pinned(samples["img_mask"]))
    tg = []
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    for i, t in enumerate(targets):
        d = dict(t, size=torch.tensor([S, S]), orig_size=torch.tensor([S, S]), image_id=torch.tensor(i))
        if masks:
            cx, cy, bw, bh = [float(v) for v in t["boxes"][0]]
            d["masks"] = ((((xx + 0.5) / S - cx).abs() < bw / 2) & (((yy + 0.5) / S - cy).abs() < bh / 2))[None]
        tg.append({k: pinned(v) for k, v in d.items()})
    return model, crit, post, [(s, tg)] * a.batches


def timed(model, crit, post, loader, switch):
    if switch is None:
        os.environ.pop("REFTR_EVAL_METRICS", None)
    else:
        os.environ["REFTR_EVAL_METRICS"] = switch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    stats, _ = evaluate(model, crit, post, loader, dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(loader), stats


for name, masks in (("REC configs[1]", False), ("REC+RES configs[3]", True)):
    model, crit, post, loader = make(masks)
    variants = [("baseline", None)] if a.as_baseline else [("metered", "1"), ("torch loop", "0")]
    ms = {v: [] for v, _ in variants}
    keys = {}
    for r in range(a.rounds + 1):                 # round 0 warms up every variant at this shape
        for v, sw in variants:
            t, stats = timed(model, crit, post, loader, sw)
            keys[v] = sorted(stats)
            if r:
                ms[v].append(t)
    for v, _ in variants:
        print("%-20s %-11s %7.3f ms/batch (median of %d runs of %d batches of %d; min %.3f max %.3f)" % (
            name, v, statistics.median(ms[v]), a.rounds, a.batches, B, min(ms[v]), max(ms[v])), flush=True)
    print(json.dumps({"shape": name, "ms_per_batch": ms, "keys": keys}), flush=True)
    del model, crit, post, loader
    torch.cuda.empty_cache()
