"""Backbone variants at configs[1]'s geometry (640 x 640, batch 8, L = 40, AdamW, clip 0.1, captured step) and the grouped
convolution kernels of the ResNeXt stages against F.conv2d(groups=G) (bf16, channels-last) on the same shapes.

    python benchmarks/backbones.py steps [--steps K --warmup W]      ms/step for resnet50, resnext50_32x4d, resnext101_32x8d,
                                                                      wide_resnet50_2
    python benchmarks/backbones.py kernels [--iters N]               per launch: rt_gconv forward / backward-data, rt_gconv_wgrad
                                                                      and torch's grouped conv forward / backward-data, us and GB/s
                                                                      (HIP events; run it under `rocprofv3 --kernel-trace --stats`
                                                                      for the per-kernel table)
GB/s = compulsory bytes (input read once, output written once, bf16) / time; the HBM peak is 6.3 TB/s.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["resnet50", "resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2"]


def step_ms(name, steps, warmup, B=8, S=640, L=40):
    from bench import synth_batch
    from reftr_amd.engine_vg import CapturedTrainStep
    from reftr_amd.models import layout as Lm
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.models.reftr_transformer import BACKBONES, RefTR
    from reftr_amd.optim import FusedAdamW
    from reftr_amd.util.misc import NestedTensor
    dev = torch.device("cuda", 0)
    layers, groups, wpg = BACKBONES[name]
    cfg = Lm.ModelConfig(resnet_layers=layers, resnet_groups=groups, resnet_width_per_group=wpg)
    model = RefTR(cfg, device=dev, aux_loss=True)
    wd = {"loss_giou": 1.0, "loss_bbox": 1.0}
    wd.update({f"{k}_{i}": v for i in range(cfg.dec_layers - 1) for k, v in list(wd.items())})
    crit = CriterionVGMultiPhrase(wd, ["boxes"])
    torch.manual_seed(1234)
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02)
    model.mark_dirty()
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    model.train()
    samples, targets = synth_batch(B, S, S, L, dev, 1234)
    s = {k: v.to(dev) for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].to(dev), samples["img_mask"].to(dev))
    tg = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    cap = CapturedTrainStep(model, crit, opt, 0.1, s, tg)
    sb, tb = cap.batch
    for _ in range(warmup):
        cap(sb, tb)[0].item()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = cap(sb, tb)[0].item()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    del cap, model, opt
    torch.cuda.empty_cache()
    return ms, loss


def grouped_shapes(B=8, S=640):
    """(label, B, H_in, W_in, C, G, stride) of every distinct grouped 3x3 in resnext50_32x4d and resnext101_32x8d at S x S."""
    out = []
    for name, G, wpg in (("resnext50_32x4d", 32, 4), ("resnext101_32x8d", 32, 8)):
        for li in range(4):
            C = int(64 * 2 ** li * wpg / 64) * G
            h = S // 4 // 2 ** li                           # stage output size
            if li > 0:
                out.append((f"{name} layer{li + 1}.0 s2", B, 2 * h, 2 * h, C, G, 2))
            out.append((f"{name} layer{li + 1} s1", B, h, h, C, G, 1))
    return out


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters     # us


def kernels(iters):
    from reftr_amd import hip as H
    print("%-34s %4s %6s | %9s %8s | %9s %8s | %9s %8s | %9s %8s | %9s" % (
        "shape", "Cg", "MB", "fwd us", "GB/s", "torch us", "GB/s", "dgrad us", "GB/s", "torch us", "GB/s", "wgrad us"))
    for label, B, Hh, Ww, C, G, s in grouped_shapes():
        Ho, Wo = (Hh - 1) // s + 1, (Ww - 1) // s + 1
        cg = C // G
        x = torch.randn(B * Hh * Ww, C, device="cuda").bfloat16()
        w = (torch.randn(C, 3, 3, cg, device="cuda") / (9 * cg) ** 0.5).bfloat16()
        bias = torch.zeros(C, device="cuda")
        dy = torch.randn(B * Ho * Wo, C, device="cuda").bfloat16()
        gate = torch.randn(B * Hh * Ww, C, device="cuda").bfloat16()
        dw = torch.zeros(C, 3, 3, cg, device="cuda")
        geom = (B, Hh, Ww, C, Ho, Wo, C, 3, 3, s, 1)
        geom_t = (B, Ho, Wo, C, Hh, Ww, C, 3, 3, s, 1)
        ob = torch.empty(B * Ho * Wo, C, device="cuda").bfloat16()
        oi = torch.empty(B * Hh * Ww, C, device="cuda").bfloat16()
        t_f = timed(lambda: H.gconv(x, w, geom=geom, groups=G, bias=bias, act=H.ACT_RELU, out_bf16=ob), iters)
        t_d = timed(lambda: H.gconv(dy, w, geom=geom_t, groups=G, transposed=True, gate=gate, out_bf16=oi), iters)
        t_w = timed(lambda: H.gconv_wgrad(dy, x, dw, geom=geom, groups=G, overwrite=True), iters)
        # torch / MIOpen: bf16 channels-last NCHW views of the same tensors
        xt = x.view(B, Hh, Ww, C).permute(0, 3, 1, 2)
        wt = w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        dyt = dy.view(B, Ho, Wo, C).permute(0, 3, 1, 2)
        t_tf = timed(lambda: F.conv2d(xt, wt, None, s, 1, 1, G), iters)
        t_td = timed(lambda: torch.ops.aten.convolution_backward(dyt, xt, wt, None, (s, s), (1, 1), (1, 1), False, (0, 0), G,
                                                                  (True, False, False)), iters)
        fb = 2.0 * (B * Hh * Ww * C + B * Ho * Wo * C)        # fwd: x in, y out;  dgrad: dy in, dx out (+ the gate read)
        db = fb + 2.0 * B * Hh * Ww * C
        print("%-34s %4d %6.0f | %9.1f %8.0f | %9.1f %8.0f | %9.1f %8.0f | %9.1f %8.0f | %9.1f" % (
            label, cg, fb / 1e6, t_f, fb / t_f / 1e3, t_tf, fb / t_tf / 1e3, t_d, db / t_d / 1e3, t_td, fb / t_td / 1e3, t_w))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["steps", "kernels"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--names", default=",".join(NAMES))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from reftr_amd import hip as H
    H.lib()
    if a.what == "steps":
        for name in a.names.split(","):
            ms, loss = step_ms(name, a.steps, a.warmup)
            print(f"{name:20s} {ms:8.2f} ms/step  ({8e3 / ms:6.1f} img/s, loss {loss:.4f})")
            sys.stdout.flush()
    else:
        kernels(a.iters)


if __name__ == "__main__":
    main()
