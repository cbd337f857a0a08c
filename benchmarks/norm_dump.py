"""Bit-level record of rt_layernorm_fwd / rt_layernorm_bwd, for comparing two builds of the library.

    python benchmarks/norm_dump.py OUTDIR
    python benchmarks/norm_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of cases through hip.layernorm_fwd / hip.layernorm_bwd.  Per case it writes
OUTDIR/<case>.<array>.bin (raw fp32, bf16 as uint16) and one line "<case> <kernels> <sha256 of each array of ARRAYS>" in
OUTDIR/hashes.txt.  Parameter gradients go through the partial-sum path (LnGradBatch: a fixed summation order); the `atomics` cases
have M = 4, one workgroup, so every channel receives a single add into zero and there is no order to depend on.

The second form takes two runs of the base build and one of the new build: the two base runs must agree, and every case of the new
run must equal them byte for byte.  Exit status 1 on any difference and on any case that one of the runs lacks.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARRAYS = ("y_f32", "y_bf16", "ypos_bf16", "mean", "rstd", "dx_f32", "dx_bf16", "dgamma", "dbeta")
# name, M, D, act, drop_p, drop2_p, dy2, rowmap (rows per group, group stride, offset) or None, parameter gradients: "partials" | "atomics"
# D = 256 / 768: the vectorised kernels, D = 100 / 1024: the generic ones.  M = 1029 > 4 * 256 workgroups: a wave walks a second row;
# M = 3525: one row past the 880 workgroups of the partial-sum path.
CASES = [
    ("vec256_plain", 37, 256, 0, 0.0, 0.0, False, None, "partials"),
    ("vec256_relu_dy2", 5, 256, 1, 0.0, 0.0, True, None, "partials"),
    ("vec256_all", 1029, 256, 1, 0.1, 0.2, True, (343, 350, 2), "partials"),
    ("vec256_cap", 3525, 256, 0, 0.1, 0.0, False, None, "partials"),
    ("vec256_atomics", 4, 256, 1, 0.1, 0.2, True, None, "atomics"),
    ("vec768_plain", 50, 768, 0, 0.0, 0.0, False, None, "partials"),
    ("vec768_all", 321, 768, 1, 0.1, 0.2, True, (107, 110, 1), "partials"),
    ("vec768_atomics", 4, 768, 0, 0.0, 0.2, True, None, "atomics"),
    ("gen100_plain", 37, 100, 0, 0.0, 0.0, False, None, "partials"),
    ("gen100_all", 321, 100, 1, 0.1, 0.2, True, (107, 110, 1), "partials"),
    ("gen100_atomics", 4, 100, 1, 0.1, 0.0, False, None, "atomics"),
    ("gen1024_plain", 13, 1024, 0, 0.0, 0.0, True, None, "partials"),
    ("gen1024_all", 1029, 1024, 1, 0.1, 0.2, True, (343, 350, 2), "partials"),
    ("gen1024_atomics", 4, 1024, 1, 0.1, 0.2, True, None, "atomics"),
]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_all(outdir):
    import torch
    from reftr_amd import hip
    os.makedirs(outdir, exist_ok=True)
    hip.set_seed_dev(None)
    lines = []
    for ci, (name, M, D, act, drop_p, drop2_p, use_dy2, rowmap, pg) in enumerate(CASES):
        g = torch.Generator().manual_seed(3000 + ci)
        rows = M if rowmap is None else (M // rowmap[0]) * rowmap[1]          # rows of the mapped (sequence) buffers
        x = torch.randn(M, D, generator=g).cuda()
        gam = (torch.rand(D, generator=g) + 0.5).cuda()
        bet = (torch.randn(D, generator=g) * 0.1).cuda()
        pos, dy = torch.randn(rows, D, generator=g).cuda(), torch.randn(rows, D, generator=g).cuda()
        dy2 = torch.randn(rows, D, generator=g).cuda() if use_dy2 else None
        yf = torch.zeros(rows, D, device="cuda")
        yb, ypb = torch.zeros(rows, D, device="cuda", dtype=torch.bfloat16), torch.zeros(rows, D, device="cuda", dtype=torch.bfloat16)
        rm = rowmap or (0, 0, 0)
        _, _, _, mean, rstd = hip.layernorm_fwd(x, gam, bet, 1e-5, act=act, drop_p=drop_p, drop_seed=11 + ci, pos=pos, y_f32=yf, y_bf16=yb,
                                                ypos_bf16=ypb, rowmap=rm)
        dgam, dbet = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        batch = hip.LnGradBatch() if pg == "partials" else None
        dxf, dxb = hip.layernorm_bwd(dy, x, gam, bet, mean, rstd, dgam, dbet, dy2=dy2, act=act, drop_p=drop_p, drop_seed=11 + ci,
                                     drop2_p=drop2_p, drop2_seed=101 + ci, rowmap=rm, pg_batch=batch)
        if batch is not None:
            batch.run()
        torch.cuda.synchronize()
        hs = []
        for key, t in zip(ARRAYS, (yf, yb, ypb, mean, rstd, dxf, dxb, dgam, dbet)):
            a = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
            a = a.view(np.uint16) if a.dtype == np.int16 else a
            a.tofile(os.path.join(outdir, f"{name}.{key}.bin"))
            hs.append(sha(a))
        lines.append(f"{name} {'vec' if D in (256, 768) else 'generic'}/{pg} " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_hashes(d):
    return {l.split()[0]: l.split()[1:] for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    want = [c[0] for c in CASES]
    rows, bad, unstable = [], 0, 0
    for case in want:
        if any(case not in h or len(h[case]) != 1 + len(ARRAYS) for h in (h1, h2, hn)):
            bad += 1
            rows.append(f"{case:18s} MISSING from " + " ".join(n for n, h in (("base1", h1), ("base2", h2), ("new", hn)) if case not in h or len(h[case]) != 1 + len(ARRAYS)))
            continue
        route, *hs = h1[case]
        stable = h2[case][1:] == hs
        same = [a == b for a, b in zip(hs, hn[case][1:])]
        ok = stable and all(same)
        verdict = "equal" if ok else "BASE RUNS DIFFER" if not stable else "DIFFERENT: " + " ".join(k for k, s in zip(ARRAYS, same) if not s)
        bad += not ok
        unstable += not stable
        rows.append(f"{case:18s} {route:17s} " + " ".join(f"{a[:8]}/{b[:8]}" for a, b in zip(hs, hn[case][1:])) + f" {verdict}")
    extra = sorted((set(h1) | set(h2) | set(hn)) - set(want))
    bad += len(extra)
    text = "sha256 (first 8 digits) of every array, base build / new build\n" + \
        f"{'case':18s} {'kernels/grads':17s} " + " ".join(f"{k:17s}" for k in ARRAYS) + " verdict\n" + "\n".join(rows) + \
        "".join(f"\n{c}: not a case of this tool" for c in extra) + \
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
