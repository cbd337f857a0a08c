"""Bit-level record of the optimizer-side launches of rt_optim.hip and rt_zero_chunks, for comparing two builds of the library.

    python benchmarks/optim_dump.py OUTDIR
    python benchmarks/optim_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of small cases through reftr_amd.hip: rt_adamw_flat / rt_sgd_flat (fp32 and bf16 gradients, two
spans, device step and learning rates, active == 0), rt_adamw_mat + rt_adamw_chunks over the synthetic buffer of
test_matrix_adamw_equals_flat_adamw_plus_weight_prep (and rt_adamw_flat over the same buffer: the `matflat` cases), a sparse-state matrix
job, rt_sqnorm / rt_sqnorm_bf16, rt_sqnorm_finish / rt_round_chunks / rt_zero_chunks over a ragged chunk table, rt_grad_accum,
rt_finish_step / rt_finish_stats / rt_counter_add, and one M = 8 hip.linear_wgrad into a registered matrix, which reaches rt_sq_pass and
rt_round_pass (the passes around the launches that do not account for themselves; the matrix is registered the way benchmarks/wgrad_dump.py
and tests/test_grouped_conv_gpu.py do it, by an entry (weakref to an owner, slots / twin address) in hip._SQACC_MAP / hip._G16_MAP -- the
tables behind ParamStore.register_overwritable and reftr_amd.parallel: if their layout changes, this case changes with them).  Per case it writes OUTDIR/<case>.<array>.bin and one
line "<case> <array>=<sha256> ..." in OUTDIR/hashes.txt.

Every case is deterministic by construction: gnorm_sq is computed on the host and passed in, the norm kernels run at one workgroup or at
one add per accumulator slot (at most 256 chunks / pieces; the accumulating wgrad case adds -|before|^2 and +|after|^2 to a slot from
two launches that the stream orders).

The second form takes two runs of the base build and one of the new build: the two base runs must agree, and every array of the new
run must equal them byte for byte.  A flat AdamW case that differs from the base is accepted only if the new build's flat pass equals
its own rt_adamw_mat + rt_adamw_chunks byte for byte on the synthetic buffer; the table then states its largest distance from the base.
The table also says, for both builds, whether flat == mat + chunks there.  Exit status 1 on any other difference and on a missing case.
"""
import hashlib
import os
import sys
import weakref

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = [(0, 1), (5, 3), (12, 5), (4097, 16384), (20484, 16384), (36870, 1023)]      # the table of test_chunk_table_kernels_at_ragged_offsets
FLAT_ADAMW = ("flat_fp32", "flat_g16", "flat_spans", "flat_devwords", "flat_idle")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class _Owner:
    pass


def cases():
    """Yields (case, {array: tensor})."""
    import torch
    from reftr_amd import hip
    from reftr_amd.optim import cover_span
    dev = "cuda"

    def gen(seed):
        return torch.Generator().manual_seed(seed)

    # ---- the flat passes
    g = gen(4000)
    n = 3 * 4096 + 8
    p0 = torch.randn(n, generator=g).to(dev); gr = (torch.randn(n, generator=g) * 0.1).to(dev)
    m0 = (torch.randn(n, generator=g) * 0.01).to(dev); v0 = (torch.rand(n, generator=g) * 1e-3).to(dev)
    g16 = gr.bfloat16()
    ranges = [(0, 4096, 1e-3, 1e-4), (4096, n, 1e-4, 0.0)]

    def sq_of(t):
        return (t.double() ** 2).sum().float().reshape(1).to(dev)

    def flat(spans=(None,), sgd=False, src=gr, **kw):
        p, m, v, gn = p0.clone(), m0.clone(), v0.clone(), torch.zeros(1, device=dev)
        rg = kw.pop("ranges", ranges)
        for sp in spans:
            hip.adamw_flat(p, gr, m, v if not sgd else m[:4], step=3, ranges=rg, gnorm_sq=sq_of(src), gnorm_out=gn,
                           grad_scale=0.5, max_norm=0.1, span=sp, sgd=sgd, **kw)
        return dict(p=p, m=m, gn=gn) if sgd else dict(p=p, m=m, v=v, gn=gn)

    yield "flat_fp32", flat()
    yield "flat_g16", flat(src=g16, g16=g16)
    yield "flat_spans", flat(spans=((0, 4100), (4100, n)))
    lr_dev = torch.tensor([1e-3, 1e-4, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    yield "flat_devwords", flat(ranges=[(0, 4096, 7.0, 1e-4), (4096, n, 9.0, 0.0)], lr_dev=lr_dev,
                                step_dev=torch.tensor([5], dtype=torch.int32, device=dev))
    yield "flat_idle", flat(active=torch.zeros(1, dtype=torch.int32, device=dev))
    whole = cover_span([], 0, n)[2]                     # the chunk kernel alone over the same buffer: what flat_fp32 / flat_g16 got?
    ctab = torch.tensor(whole, dtype=torch.int64).to(dev)
    yield "chunks_fp32", flat(chunks=(ctab, len(whole) // 2))
    yield "chunks_g16", flat(src=g16, g16=g16, chunks=(ctab, len(whole) // 2))
    yield "sgd_fp32", flat(sgd=True, beta1=0.9)
    yield "sgd_g16", flat(sgd=True, beta1=0.9, src=g16, g16=g16)

    # ---- rt_adamw_mat + rt_adamw_chunks over the synthetic buffer of test_matrix_adamw_equals_flat_adamw_plus_weight_prep
    g = gen(4001)
    mats = [(256, 192, 1, 128), (256 + 192 * 128 + 40, 72, 9, 64), (256 + 192 * 128 + 40 + 72 * 9 * 64 + 8, 10, 1, 12)]
    nb = (mats[-1][0] + 10 * 12 + 4096 + 36 + 3) // 4 * 4
    pb = torch.randn(nb, generator=g).to(dev); gb = (torch.randn(nb, generator=g) * 0.1).to(dev)
    mb = (torch.randn(nb, generator=g) * 0.01).to(dev); vb = (torch.rand(nb, generator=g) * 1e-3).to(dev)
    scale = (torch.rand(72, generator=g) + 0.5).to(dev)
    rb = [(0, 24840, 1e-3, 1e-4), (24840, nb, 1e-4, 0.0)]
    jobs, tiles, chunks = cover_span(mats, 0, nb)
    ctab = torch.tensor(chunks, dtype=torch.int64).to(dev)
    for tag, extra, src in (("fp32", {}, gb), ("g16", dict(g16=gb.bfloat16()), gb.bfloat16())):
        kw = dict(step=3, ranges=rb, gnorm_sq=sq_of(src), grad_scale=0.5, max_norm=0.1, **extra)
        p, m, v, gn = pb.clone(), mb.clone(), vb.clone(), torch.zeros(1, device=dev)
        out, rows = {}, []
        for i, (off, N, T, C, first) in enumerate(jobs):
            W = torch.zeros(N, T, C, dtype=torch.bfloat16, device=dev); WT = torch.zeros(C, T, N, dtype=torch.bfloat16, device=dev)
            rows.append([off, scale.data_ptr() if i == 1 else 0, W.data_ptr(), WT.data_ptr(), N, T, C, first])
            out[f"W{i}"], out[f"WT{i}"] = W, WT
        tab = torch.tensor(rows, dtype=torch.int64).to(dev)
        hip.adamw_flat(p, gb, m, v, gnorm_out=gn, mat=(tab, len(rows), tiles), chunks=(ctab, len(chunks) // 2), **kw)
        yield "mat_" + tag, dict(p=p, m=m, v=v, gn=gn, **out)
        p, m, v, gn = pb.clone(), mb.clone(), vb.clone(), torch.zeros(1, device=dev)
        hip.adamw_flat(p, gb, m, v, gnorm_out=gn, **kw)
        yield "matflat_" + tag, dict(p=p, m=m, v=v, gn=gn)

    # ---- a sparse-state job, as in test_sparse_state_adamw_is_bit_exact_and_skips_untouched_pieces (the skip is taken)
    g = gen(4002)
    N, K = 100, 768
    kt = (K + 255) // 256
    p = torch.randn(N * K, generator=g).to(dev); m = torch.zeros(N * K, device=dev); v = torch.zeros(N * K, device=dev)
    flags = torch.ones(N * kt, dtype=torch.uint8, device=dev)
    tab = torch.tensor([[0, flags.data_ptr(), 0, 0, N, 1, K, 0]], dtype=torch.int64).to(dev)
    for step, rows in enumerate(([3, 50], [3], [], [77, 50]), start=1):
        gs = torch.zeros(N, K)
        for r in rows:
            gs[r] = torch.randn(K, generator=g) * 0.1
        if step == 4:
            gs[12, 300:310] = 0.5
        gs = gs.reshape(-1).to(dev)
        hip.adamw_flat(p, gs, m, v, step=step, ranges=[(0, N * K, 1e-5, 1e-4)], gnorm_sq=sq_of(gs), max_norm=0.1,
                       mat=(tab, 1, ((N + 31) // 32) * kt))
    yield "mat_sparse", dict(p=p, m=m, v=v, flags=flags)

    # ---- rt_sqnorm: one workgroup each, tails included
    g = gen(4003)
    out = torch.zeros(1, device=dev)
    hip.sqnorm(torch.randn(1000, generator=g).to(dev), out)
    yield "sqnorm_fp32", dict(out=out)
    out = torch.zeros(1, device=dev)
    hip.sqnorm(torch.randn(2043, generator=g).to(dev).bfloat16(), out)
    yield "sqnorm_bf16", dict(out=out)

    # ---- the ragged chunk table: one add per slot
    g = gen(4004)
    base = torch.randn(45056, generator=g).to(dev)
    tab = torch.tensor([x for c in CHUNKS for x in c], dtype=torch.int64).to(dev)
    slots = torch.zeros(hip.SQ_SLOTS * hip.SQ_STRIDE, device=dev); out = torch.zeros(1, device=dev)
    hip.sqnorm_finish(base, tab, len(CHUNKS), slots, out, extra=torch.tensor([3.5], device=dev))
    twin = torch.full((45056,), 7.0, dtype=torch.bfloat16, device=dev)
    hip.round_chunks(base, twin, tab, len(CHUNKS))
    z = base.clone()
    hip.zero_chunks(z, tab, len(CHUNKS))
    yield "chunk_table", dict(sq=out, slots=slots, twin=twin, zeroed=z)

    # ---- rt_grad_accum: aligned, and g one element off alignment (head == n)
    g = gen(4005)
    na = 3 * 4096 + 5
    for tag, shift in (("aligned", 0), ("misaligned", 1)):
        gbuf = torch.randn(na + 1, generator=g).to(dev)
        gg = gbuf[shift:shift + na]
        acc = torch.zeros(na, device=dev)
        hip.grad_accum(hip.ACCUM_FIRST, gg, acc)
        first = acc.clone()
        gg.mul_(0.5)
        hip.grad_accum(hip.ACCUM_ADD, gg, acc)
        added = acc.clone()
        ws = torch.zeros(hip.GRAD_ACCUM_SLOTS, device=dev); sq = torch.zeros(1, device=dev)
        hip.grad_accum(hip.ACCUM_FINISH, gg, acc, scale=1.0 / 3, partials=ws, out_sq=sq)
        yield "grad_accum_" + tag, dict(first=first, added=added, g=gg.clone(), sq=sq)

    # ---- the scalar launches
    rec = {}
    i32 = lambda x: torch.tensor([x], dtype=torch.int32, device=dev)
    for tag, word, loss_val in (("good", 0, 2.0), ("veto", 3, 2.0), ("nan", 0, float("nan"))):
        step, active, loss = i32(7), i32(1), torch.tensor([loss_val], device=dev)
        hip.finish_step(step, active, i32(word), loss)
        rec[f"step_{tag}"] = torch.cat([step, active])
        step, active, gn, stats = i32(7), i32(1), torch.zeros(1, device=dev), torch.full((4,), -1.0, device=dev)
        srcs = [torch.tensor([0.125], device=dev), torch.tensor([7.0], device=dev)]
        hip.finish_stats(step, active, i32(word), loss, torch.tensor([6.25], device=dev), 0.5, gn, srcs=srcs, cond_in_stats=True, stats=stats)
        rec[f"stats_{tag}"] = torch.cat([step.float(), active.float(), gn, stats])
    c = i32(4); hip.counter_add(c, 3); rec["counter_plain"] = c
    c = i32(4); hip.counter_add(c, 3, unless=i32(0)); rec["counter_unless_0"] = c
    c = i32(4); hip.counter_add(c, 3, unless=i32(2)); rec["counter_unless_set"] = c
    c = i32(4); hip.counter_add(c, 3, unless=i32(2), reset_else=True); rec["counter_reset_else"] = c
    yield "scalars", rec

    # ---- rt_sq_pass / rt_round_pass: an M = 8 Linear weight gradient into a registered matrix (2 pieces, one of them short)
    g = gen(4006)
    M, N, K = 8, 72, 80
    dy = torch.randn(M, N, generator=g).to(dev).bfloat16(); x = torch.randn(M, K, generator=g).to(dev).bfloat16()
    dw0 = (torch.randn(N, K, generator=g) * 0.5).to(dev)
    for tag, ow in (("accumulate", False), ("overwrite", True)):
        owner = _Owner()
        dw = dw0.clone(); slots = torch.zeros(hip.SQ_SLOTS * hip.SQ_STRIDE, device=dev)
        twin = torch.zeros(N * K, dtype=torch.bfloat16, device=dev)
        hip._SQACC_MAP[dw.data_ptr()] = (weakref.ref(owner), slots)
        hip._G16_MAP[dw.data_ptr()] = (weakref.ref(owner), twin.data_ptr())
        try:
            hip.linear_wgrad(dy, x, dw, overwrite=ow)
            torch.cuda.synchronize()
        finally:
            hip._SQACC_MAP.pop(dw.data_ptr(), None); hip._G16_MAP.pop(dw.data_ptr(), None)
        yield "wgrad_passes_" + tag, dict(dw=dw, slots=slots, twin=twin)


def run_all(outdir):
    import torch
    os.makedirs(outdir, exist_ok=True)
    lines = []
    for case, arrays in cases():
        torch.cuda.synchronize()
        hs = []
        for key, t in arrays.items():
            a = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
            a.tofile(os.path.join(outdir, f"{case}.{key}.bin"))
            hs.append(f"{key}={sha(a)}")
        lines.append(case + " " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_hashes(d):
    return {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def flat_is_chunks(h):
    return all(h[f"flat_{t}"] == h[f"chunks_{t}"] for t in ("fp32", "g16") if f"flat_{t}" in h and f"chunks_{t}" in h)


def flat_is_matchunks(h):
    return all(h[f"matflat_{t}"][k] == h[f"mat_{t}"][k] for t in ("fp32", "g16") for k in ("p", "m", "v", "gn")
               if f"matflat_{t}" in h and f"mat_{t}" in h)


def distance(d1, d2, case, keys):
    """largest |a - b| / max |a| over the fp32 arrays `keys` of a case in two runs"""
    worst = 0.0
    for k in keys:
        a = np.fromfile(os.path.join(d1, f"{case}.{k}.bin"), dtype=np.float32); b = np.fromfile(os.path.join(d2, f"{case}.{k}.bin"), dtype=np.float32)
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max() / max(float(np.abs(a).max()), 1e-30)))
    return worst


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    want = list(h1)
    rows, bad, unstable = [], 0, 0
    new_flat_ok = flat_is_matchunks(hn)
    for case in want:
        if case not in h2 or case not in hn or set(h2[case]) != set(h1[case]) or set(hn[case]) != set(h1[case]):
            bad += 1
            rows.append(f"{case:22s} MISSING (or other arrays) in a run")
            continue
        stable = h2[case] == h1[case]
        diff = [k for k in h1[case] if hn[case][k] != h1[case][k]]
        ok = stable and not diff
        verdict = "equal" if ok else "BASE RUNS DIFFER" if not stable else "DIFFERENT: " + " ".join(diff)
        if stable and diff and (case in FLAT_ADAMW or case.startswith("matflat_")):
            d = distance(base1, new, case, diff)
            ok = new_flat_ok and d <= 2e-7
            verdict = f"DIFFERENT: {' '.join(diff)} (largest distance from the base {d:.3g} relative)" + \
                ("; the new flat pass equals the new mat + chunks" if new_flat_ok else "")
        bad += not ok
        unstable += not stable
        rows.append(f"{case:22s} " + " ".join(f"{k}:{h1[case][k][:8]}/{hn[case][k][:8]}" for k in h1[case]) + f"  {verdict}")
    extra = sorted((set(h2) | set(hn)) - set(want))
    bad += len(extra)
    text = "sha256 (first 8 digits) of every array, base build / new build\n" + "\n".join(rows) + \
        "".join(f"\n{c}: not a case of the base run" for c in extra) + \
        f"\nrt_adamw_flat == rt_adamw_mat + rt_adamw_chunks byte for byte on the synthetic buffer (p, m, v, norm; fp32 and bf16 gradients): " \
        f"base build {'yes' if flat_is_matchunks(h1) else 'no'}, new build {'yes' if new_flat_ok else 'no'}" + \
        f"\nrt_adamw_flat == rt_adamw_chunks alone over the flat cases' buffer: base build {'yes' if flat_is_chunks(h1) else 'no'}, " \
        f"new build {'yes' if flat_is_chunks(hn) else 'no'}" + \
        f"\n{len(want)} cases, {unstable} not reproduced by the base build itself, {bad} failed\n"
    print(text)
    if table:
        with open(table, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--compare" in sys.argv:
        table = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else None
        if table in args:
            args.remove(table)
        sys.exit(compare(args[0], args[1], args[2], table))
    run_all(args[0])
