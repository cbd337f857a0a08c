"""Bit-level record of the image side -- input staging (rt_input.hip, rt_raw_stage.hip), the stem and weight prep (rt_backbone.hip) -- for
comparing two builds of the library, and a captured-graph timing of the two launches no other benchmark times.

    python benchmarks/input_dump.py OUTDIR
    python benchmarks/input_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]
    python benchmarks/input_dump.py --time [--runs 5]

The first form runs a fixed, seeded list of cases through the hip.* wrappers and BatchCanvas.stage and writes one line
"<case> <array>=<sha256> ..." per case to OUTDIR/hashes.txt.  The batches are those of tests/test_raw_stage_gpu.py and
tests/test_batch_stage_gpu.py (imported from there), the weight-prep jobs those of tests/test_gemm_gpu.py::test_weight_prep_batched.

The second form takes two runs of the base build and one of the new build, each from a fresh process.  None of these kernels uses an
atomic: every array must be equal in all three runs.  Exit status 1 on any difference and on any case or array that a run lacks.

The third form prints us per launch, 50 launches recorded into one hipGraph, one event pair around a replay, median of `--runs` replays
with min - max: rt_batch_stage at B = 8, 427 x 640 -> 640 x 640 with masks; the full weight-prep job table of a ResNet-50 backbone
(ResNetBody._prep_all, one rt_weight_prep_batched launch); and one rt_weight_prep call of a 3072 x 768 Linear with both copies.
"""
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RAW = [("main", [(144, 144), (141, 139)]), ("small", [(144, 144), (141, 139)]), ("nearest", [(180, 180), (183, 181)])]
BATCH_STAGE = [("c8x12", (8, 12), 3, (5, 7), (0, 3, 1), [(8, 12), (5, 7), (1, 1)], 1), ("c7x10", (7, 10), 3, (5, 7), (0, 3, 1), [(7, 10), (5, 7), (1, 1)], 1),
               ("c640", (640, 640), 8, (427, 640), (1,) * 8, [(427, 640)] * 8, 0)]
CHAIN = [(375, 500, 240, 320), (97, 211, 147, 320)]                  # two sizes of tests/test_input_pipeline.py at size = max_size = 320
STEM = [(2, 70, 52), (3, 33, 47), (1, 17, 16)]
PREP = [(24, 9, 16, True), (100, 1, 70, False), (4, 1, 256, False), (33, 4, 33, True), (768, 1, 3072, False), (136, 9, 72, True),
        (72, 1, 100, True), (100, 1, 72, False)]


def case_names():
    return ([f"raw_{n}_{h}x{w}" for n, cvs in RAW for h, w in cvs] + [f"batch_stage_{c[0]}" for c in BATCH_STAGE]
            + [f"chain_{h}x{w}" for h, w, _, _ in CHAIN] + [f"stem_{b}x{h}x{w}" for b, h, w in STEM]
            + [f"prep_{k}_{n}x{t}x{c}" for k in ("single", "batched") for n, t, c, _ in PREP])


def staged_arrays(st):
    d = dict(img=st.samples["img"].tensors, mask=st.samples["img"].mask, boxes=st.targets_static[0], tgt_off=st.targets_static[1],
             num_boxes=st.targets_static[2])
    if st.tgt_masks is not None:
        d["tgt_masks"] = st.tgt_masks
    return d


def cases():
    """Yields (case name, {array name: tensor}); needs a GPU."""
    import torch
    import test_batch_stage_gpu as TB
    import test_raw_stage_gpu as TR
    from reftr_amd import hip
    from reftr_amd.data import DeviceInputPipeline
    from reftr_amd.data.canvas import BatchCanvas
    from reftr_amd.data.device_input import MEAN, STD

    for name, canvases in RAW:
        _, _, s, t = TR.make(**getattr(TR, name.upper()))
        for h, w in canvases:
            yield f"raw_{name}_{h}x{w}", staged_arrays(BatchCanvas(h, w, 3, masks=True).stage(s, t))

    for name, canvas, B, src, counts, mask_hw, offset in BATCH_STAGE:
        s, t = TB.make_batch(B, *src, counts, mask_hw=mask_hw, offset=offset)
        yield f"batch_stage_{name}", staged_arrays(BatchCanvas(*canvas, max(counts), masks=True).stage(s, t))

    pipe = DeviceInputPipeline(size=320, max_size=320)
    for i, (h, w, oh, ow) in enumerate(CHAIN):
        img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5000 + i)).cuda()
        resized = pipe.resize(img, oh, ow)
        batch, mask = hip.img_collate_norm([resized, resized[: oh // 2, : ow // 3].contiguous()], oh + 3, ow + 5, MEAN, STD)
        yield f"chain_{h}x{w}", dict(resized=resized, batch=batch, mask=mask)

    for B, H, W in STEM:
        g = torch.Generator().manual_seed(B * 100 + H)
        img = torch.randn(B, 3, H, W, generator=g).cuda()
        w = (torch.randn(64, 7, 7, 3, generator=g) / 12).cuda()
        scale = (torch.rand(64, generator=g) + 0.5).cuda(); shift = (torch.randn(64, generator=g) * 0.3).cuda()
        Ho, Wo, _, _ = hip.stem_geometry(H, W)
        xp = hip.img_pack(img)
        wk = torch.empty(64, 7, 8, 4, dtype=torch.bfloat16, device="cuda")
        hip.stem_weight_prep(w, scale, wk)
        conv = hip.stem_conv(xp, wk, shift, Ho, Wo)
        yield f"stem_{B}x{H}x{W}", dict(xp=xp, wk=wk, conv=conv, pooled=hip.maxpool3x3s2(conv), stem_pool=hip.stem_pool(xp, wk, shift, Ho, Wo))

    g = torch.Generator().manual_seed(12)
    jobs = []
    for N, T, C, scaled in PREP:
        src = torch.randn(N, T, C, generator=g).cuda()
        jobs.append((N, T, C, src, (torch.rand(N, generator=g) + 0.5).cuda() if scaled else None))
    for kind in ("single", "batched"):
        outs, batch = [], hip.WeightPrepBatch("cuda")
        for N, T, C, src, sc in jobs:
            dst = torch.zeros(N, T, C, dtype=torch.bfloat16, device="cuda"); dst_t = torch.zeros(C, T, N, dtype=torch.bfloat16, device="cuda")
            if kind == "single":
                hip.weight_prep(src, N, T, C, scale=sc, dst=dst, dst_t=dst_t)
            else:
                batch.add(src, N, T, C, scale=sc, dst=dst, dst_t=dst_t)
            outs.append((f"prep_{kind}_{N}x{T}x{C}", dict(dst=dst, dst_t=dst_t)))
        batch.run()
        yield from outs


def run_all(outdir):
    import torch
    os.makedirs(outdir, exist_ok=True)
    lines = []
    for name, arrays in cases():
        torch.cuda.synchronize()
        hs = [f"{k}={hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()}" for k, t in arrays.items()]
        lines.append(name + " " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_hashes(d):
    return {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    want = case_names()
    rows, bad, n_arrays = [], 0, 0
    for case in want:
        lacking = [n for n, h in (("base1", h1), ("base2", h2), ("new", hn)) if case not in h or not h[case] or set(h[case]) != set(h1.get(case, {}))]
        if lacking:
            bad += 1
            rows.append(f"{case:30s} MISSING or incomplete in " + " ".join(lacking))
            continue
        for key, hv in h1[case].items():
            n_arrays += 1
            same = h2[case][key] == hv and hn[case][key] == hv
            bad += not same
            rows.append(f"{case:30s} {key:10s} {hv[:8]}/{h2[case][key][:8]}/{hn[case][key][:8]} {'equal' if same else 'DIFFERENT'}")
    extra = sorted((set(h1) | set(h2) | set(hn)) - set(want))
    bad += len(extra)
    text = "sha256 (first 8 digits) of every array: base build run 1 / base build run 2 / new build\n" + \
        f"{'case':30s} {'array':10s} {'base1/base2/new':26s} verdict\n" + "\n".join(rows) + \
        "".join(f"\n{c}: not a case of this tool" for c in extra) + f"\n{len(want)} cases, {n_arrays} arrays, {bad} failed\n"
    print(text)
    if table:
        with open(table, "w") as f:
            f.write(text)
    return 1 if bad else 0


def time_all(runs, calls=50):
    import torch
    import test_batch_stage_gpu as TB
    from oracle import reftr_oracle as O
    from oracle.shapes import param_shapes
    from oracle.weights import formula_state
    from reftr_amd import hip
    from reftr_amd.data.canvas import BatchCanvas
    from reftr_amd.models import layout as L
    from reftr_amd.models.reftr_transformer import RefTR

    def graph_us(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        g.replay(); torch.cuda.synchronize()
        out = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record(); e1.synchronize()
            out.append(e0.elapsed_time(e1) / calls * 1e3)
        return f"{statistics.median(out):8.2f} us (min {min(out):.2f} - max {max(out):.2f})"

    cv = BatchCanvas(640, 640, 1, masks=True)
    s, t = TB.make_batch(8, 427, 640, (1,) * 8, mask_hw=[(427, 640)] * 8)
    dst = cv.stage(s, t)
    print("rt_batch_stage B=8 427x640 -> 640x640, masks     ", graph_us(lambda: cv.stage(s, t, out=dst, tokens=False)), flush=True)
    model = RefTR(L.ModelConfig(enc_layers=1, dec_layers=1, bert=L.BertConfig(layers=1)), device="cuda:0")
    model.load_state_dict(formula_state(param_shapes(O.Cfg(enc_layers=1, dec_layers=1, bert=O.BertCfg(layers=1)))))
    model.body.refresh(True)
    prep = model.body._prep_all
    print(f"ResNet-50 weight-prep table, {len(prep.jobs)} jobs, {prep.tiles} tiles", graph_us(prep.run), flush=True)
    N, C = 3072, 768
    src = torch.randn(N, 1, C, device="cuda"); w = torch.empty(N, C, dtype=torch.bfloat16, device="cuda"); wt = torch.empty(C, N, dtype=torch.bfloat16, device="cuda")
    print("rt_weight_prep 3072 x 768, both copies            ", graph_us(lambda: hip.weight_prep(src, N, 1, C, dst=w, dst_t=wt)), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--time" in sys.argv:
        time_all(int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5)
    elif "--compare" in sys.argv:
        table = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else None
        if table in args:
            args.remove(table)
        sys.exit(compare(args[0], args[1], args[2], table))
    else:
        run_all(args[0])
