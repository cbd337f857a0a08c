"""What gradient accumulation costs at configs[1] (R50, 640 x 640, B = 8, L = 40, aux loss, dropout on, clip 0.1, AdamW), on a
resident batch through engine_vg.captured_train_step:

  * ms per plain step (accum_steps = 1: the deferred-AdamW graph bench.py times);
  * ms per accumulating micro-step (forward + backward graph, then rt_grad_accum first / add) and per finishing micro-step
    (the same graph, then rt_grad_accum finish + clip + AdamW), each timed launch-to-idle;
  * rt_grad_accum's achieved GB/s in each mode over the model's whole gradient buffer, beside rt_adamw_flat's on the same buffers.

    python benchmarks/accum_throughput.py [--steps 30] [--plain-only] [--label NAME] [--out FILE]

--plain-only uses nothing this feature added, so the same file also measures a checkout from before it.  Prints one JSON line;
--out appends that line to FILE (profiles/accum_throughput.txt is the runs of both checkouts in one session, alternated)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from reftr_amd import hip as H  # noqa: E402
from reftr_amd.engine_vg import captured_train_step  # noqa: E402
from reftr_amd.models import layout as Lm  # noqa: E402
from reftr_amd.models.criterion import CriterionVGMultiPhrase  # noqa: E402
from reftr_amd.models.reftr_transformer import RefTR  # noqa: E402
from reftr_amd.optim import FusedAdamW  # noqa: E402
from reftr_amd.util.misc import NestedTensor  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def kernel_gbs(fn, nbytes, reps=200):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return nbytes * reps / (a.elapsed_time(b) * 1e-3) / 1e9


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="", help="recorded in the result line (which checkout this is)")
    ap.add_argument("--out", metavar="FILE", help="append the result line to FILE")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = Lm.ModelConfig()
    model = RefTR(cfg, device=dev, aux_loss=True)
    model.train()
    wd = {"loss_giou": 1.0, "loss_bbox": 1.0}
    wd.update({f"{k}_{i}": v for i in range(cfg.dec_layers - 1) for k, v in list(wd.items())})
    crit = CriterionVGMultiPhrase(wd, ["boxes"])
    torch.manual_seed(1234)
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02)
    model.mark_dirty()
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    samples, targets = bench.synth_batch(a.batch, a.size, a.size, 40, dev, 1234)
    s = {k: v.to(dev) for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].to(dev), samples["img_mask"].to(dev))
    targets = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    out = {"label": a.label, "workload": f"configs[1]: R50 {a.size}x{a.size} B={a.batch} L=40, resident batch, captured_train_step",
           "parameters": model.store.flat_g.numel()}

    def plain():
        captured_train_step(model, crit, s, targets, opt, None, 0.1)
    for _ in range(5):
        plain()
    assert len(model._captured_steps) == 1, "the plain step did not capture (a batch off the device runs the eager loop body)"
    out["plain_step_ms"] = median([timed(plain) for _ in range(a.steps)])
    if a.plain_only:
        emit(out, a.out)
        return

    def micro(window_end):
        captured_train_step(model, crit, s, targets, opt, None, 0.1, accum_steps=2, window_end=window_end)
    for _ in range(3):
        micro(False); micro(True)
    assert len(model._captured_steps) == 2, "the accumulating step did not capture"
    acc_ms, fin_ms = [], []
    for _ in range(a.steps):
        acc_ms.append(timed(lambda: micro(False)))
        fin_ms.append(timed(lambda: micro(True)))
    out["accumulating_micro_step_ms"] = median(acc_ms)
    out["finishing_micro_step_ms"] = median(fin_ms)

    # the kernels alone, over the whole gradient buffer
    for c in model._captured_steps.values():
        c.flush()
    st = model.store
    n = st.flat_g.numel()
    ws = torch.empty(H.GRAD_ACCUM_SLOTS, dtype=torch.float32, device=dev)
    sq = torch.zeros(1, dtype=torch.float32, device=dev)
    out["grad_accum_first_GBps"] = kernel_gbs(lambda: H.grad_accum(H.ACCUM_FIRST, st.flat_g, opt.accum), 8 * n)
    out["grad_accum_add_GBps"] = kernel_gbs(lambda: H.grad_accum(H.ACCUM_ADD, st.flat_g, opt.accum), 12 * n)
    out["grad_accum_finish_GBps"] = kernel_gbs(
        lambda: H.grad_accum(H.ACCUM_FINISH, st.flat_g, opt.accum, scale=0.5, partials=ws, out_sq=sq), 12 * n)
    st.flat_g.zero_()                                  # (a zero gradient: the update below only decays)
    out["adamw_flat_GBps"] = kernel_gbs(
        lambda: H.adamw_flat(st.flat_p, st.flat_g, opt.m, opt.v, step=1, ranges=opt._ranges(), gnorm_sq=sq), 28 * n)
    emit(out, a.out)


if __name__ == "__main__":
    main()
