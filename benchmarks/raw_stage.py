"""rt_raw_stage against the chain it replaces: one batch of raw uint8 images into a captured step's canvas buffers.

Workload: B = 8 raw 375 x 500 images at size = max_size = 640 (-> 480 x 640) on a 640 x 640 canvas, one box per image, RES target
masks (`--no-masks`: without).  Both sides run in the same process, alternated, on the same device tensors:

  raw    BatchCanvas.stage of the raw batch: ONE rt_raw_stage launch;
  chain  what the tree offers without it, from the calls that stay: hip.resample_u8 x 2 per image (device taps cached), then
         rt_img_collate_norm padded to the canvas, then DeviceInputPipeline._target per image, then BatchCanvas.stage (rt_batch_stage).

Three figures each, median of `--runs` with min - max:
  device   us per call, `--calls` calls recorded into one hipGraph after warm-up, one event pair around a replay (launch to idle).  A
           capture does not take a host -> device copy from pageable memory, and two steps of the chain make one per call:
           hip.img_collate_norm's pointer table -- here the same rt_img_collate_norm launch reads a table copied from PINNED memory --
           and _target's torch.as_tensor / torch.tensor of host lists, for which there is no such way: the captured chain is WITHOUT
           _target (boxes and masks are resized once, outside), i.e. a lower bound of the chain's device time;
  eager    us per call, `--calls` calls issued eagerly between two events: the whole chain as a user's collate would call it
           (BatchCanvas.pad_on_host's pipeline call, then stage), host launch cost included;
  host     us of host time per call to issue it (the queue never fills at this count).
`cold`: the same eager call on eight source sizes the process has not seen (one per image; the chain computes their filter taps in a
Python loop per new (in, out) length and copies them to the device; rt_raw_stage computes them in the kernel), wall time from the call
to device idle, one fresh set of sizes per run.

    python benchmarks/raw_stage.py [--runs 5] [--calls 50] [--no-masks] [--out FILE]

Acceptance (the project's convention): the slowest raw run is below the fastest chain run."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reftr_amd import hip as H  # noqa: E402
from reftr_amd.data import RawImages  # noqa: E402
from reftr_amd.data.canvas import BatchCanvas  # noqa: E402
from reftr_amd.data.device_input import MEAN, STD  # noqa: E402
from reftr_amd.util.misc import NestedTensor  # noqa: E402


def raw_batch(sizes, size, masks, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda() for h, w in sizes]
    s = {"img": RawImages(imgs, size, size), "sentence": torch.zeros(len(sizes), 40, dtype=torch.long).cuda()}
    t = []
    for h, w in sizes:
        tg = {"boxes": (torch.tensor([[0.2 * w, 0.1 * h, 0.8 * w, 0.7 * h]])).cuda(), "labels": torch.zeros(1, dtype=torch.long).cuda()}
        if masks:
            tg["masks"] = (torch.rand(1, h, w, generator=g) < 0.4).cuda()
        t.append(tg)
    return s, t


def spread(xs):
    return f"{statistics.median(xs):.1f} us (min {min(xs):.1f} - max {max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-masks", action="store_true")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, src, size, masks, n = a.batch, (375, 500), 640, not a.no_masks, a.calls
    cv = BatchCanvas(size, size, 1, masks=masks)
    s, t = raw_batch([src] * B, size, masks, 1)
    oh, ow = s["img"].out_sizes()[0]
    dst_raw, dst_chain = cv.stage(s, t), cv.stage(*cv.pad_on_host(s, t))
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(
        [dst_raw.samples["img"].tensors.view(torch.int32), dst_raw.samples["img"].mask, *dst_raw.targets_static] + ([dst_raw.tgt_masks] if masks else []),
        [dst_chain.samples["img"].tensors.view(torch.int32), dst_chain.samples["img"].mask, *dst_chain.targets_static] + ([dst_chain.tgt_masks] if masks else [])))
    assert same, "rt_raw_stage and the chain disagree"
    pipe = cv._pipes[(size, size, True)]                       # the DeviceInputPipeline pad_on_host used (its device taps are warm)

    def raw():
        cv.stage(s, t, out=dst_raw)

    def chain_eager():
        nested, tg = pipe(s["img"].images, t)
        cv.stage({"img": nested, "sentence": s["sentence"]}, tg, out=dst_chain)

    # the captured chain: the same launches, the collate's pointer table from pinned memory, the targets resized once outside
    _, tg_once = pipe(s["img"].images, t)
    tables = torch.empty((n + 5, B, 3), dtype=torch.int64, pin_memory=True)      # one per recorded call: a replay reads them again
    calls = [0]
    mean3, std3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)

    def chain_captured():
        resized = [pipe.resize(im, oh, ow) for im in s["img"].images]
        row = tables[calls[0] % (n + 5)]
        calls[0] += 1
        row.copy_(torch.tensor([[r.data_ptr(), r.shape[0], r.shape[1]] for r in resized], dtype=torch.int64))
        tab = row.to("cuda", non_blocking=True)
        batch = torch.empty((B, 3, size, size), dtype=torch.float32, device="cuda")
        mask = torch.empty((B, size, size), dtype=torch.uint8, device="cuda")
        H._call("rt_img_collate_norm", tab, batch, mask, B, size, size, mean3, std3)
        cv.stage({"img": NestedTensor(batch, mask.view(torch.bool)), "sentence": s["sentence"]}, tg_once, out=dst_chain)

    def graph_of(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                fn()
        g.replay(); torch.cuda.synchronize()
        return g

    def replay_us(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def eager_us(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        host = (time.perf_counter() - t0) / n * 1e6
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3, host

    g_raw, g_chain = graph_of(raw), graph_of(chain_captured)
    torch.cuda.synchronize()
    assert torch.equal(dst_chain.samples["img"].tensors.view(torch.int32), dst_raw.samples["img"].tensors.view(torch.int32))
    for fn in (raw, chain_eager):
        eager_us(fn)
    dev = {"raw": [], "chain": []}; eag = {"raw": [], "chain": []}; host = {"raw": [], "chain": []}
    for _ in range(a.runs):                                    # alternated
        dev["raw"].append(replay_us(g_raw)); dev["chain"].append(replay_us(g_chain))
        for name, fn in (("raw", raw), ("chain", chain_eager)):
            e, h = eager_us(fn)
            eag[name].append(e); host[name].append(h)
    # cold: eight sizes nobody has seen, a fresh set per run (wall time from the call to device idle)
    cold = {"raw": [], "chain": []}
    for r in range(a.runs):
        for k, name in enumerate(("raw", "chain")):
            sizes = [(301 + 16 * r + 2 * i + k, 401 + 16 * r + 2 * i + k) for i in range(B)]
            cs, ct = raw_batch(sizes, size, masks, 10 + r)
            assert cv.fits(cs, ct)
            fn = (lambda: cv.stage(cs, ct, out=dst_raw)) if name == "raw" else (lambda: cv.stage(*cv.pad_on_host(cs, ct), out=dst_chain))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            cold[name].append((time.perf_counter() - t0) * 1e6)
    px = size * size
    wr = B * 3 * px * 4 + B * px * (2 if masks else 1)
    rd_raw = B * src[0] * src[1] * (4 if masks else 3)
    # the captured chain: horizontal pass (read h*w*3, write h*ow*3), vertical pass (read h*ow*3, write oh*ow*3), collate (read oh*ow*3,
    # write the canvas image + mask), rt_batch_stage (read them and the resized masks, write the canvas buffers)
    mv_chain = B * (src[0] * src[1] * 3 + 2 * src[0] * ow * 3 + 2 * oh * ow * 3 + (oh * ow if masks else 0)) + 2 * (B * 3 * px * 4 + B * px) + wr
    lines = [
        f"raw_stage B={B} {src[0]}x{src[1]} -> {oh}x{ow} on a {size}x{size} canvas, masks={masks}, {n} calls, {a.runs} runs, alternated; outputs bit-identical",
        f"  device (one graph, launch to idle)  rt_raw_stage {spread(dev['raw'])}: {(wr + rd_raw) / 1e6:.1f} MB moved "
        f"({wr / 1e6:.1f} written + {rd_raw / 1e6:.1f} read), {(wr + rd_raw) / statistics.median(dev['raw']) / 1e6:.2f} TB/s",
        f"                                      chain without _target {spread(dev['chain'])}: {mv_chain / 1e6:.1f} MB moved, "
        f"{mv_chain / statistics.median(dev['chain']) / 1e6:.2f} TB/s; {2 * B + 2} launches + the table copy",
        f"  eager (launch to idle, per call)    rt_raw_stage {spread(eag['raw'])};  chain {spread(eag['chain'])}",
        f"  host time per call                  rt_raw_stage {spread(host['raw'])};  chain {spread(host['chain'])}",
        f"  cold (eight new source sizes, wall) rt_raw_stage {spread(cold['raw'])};  chain {spread(cold['chain'])}",
    ]
    for what, d in (("device", dev), ("eager", eag), ("cold", cold)):
        ok = max(d["raw"]) < min(d["chain"])
        lines.append(f"  {what}: slowest rt_raw_stage run {max(d['raw']):.1f} us vs fastest chain run {min(d['chain']):.1f} us -> "
                     + ("rt_raw_stage faster in every run" if ok else "NOT separated"))
    for line in lines:
        print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if max(dev["raw"]) < min(dev["chain"]) else 1


if __name__ == "__main__":
    sys.exit(main())
