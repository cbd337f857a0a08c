"""Bit-level record of every weight-gradient route, for comparing two builds of the library.

    python benchmarks/wgrad_dump.py OUTDIR [--ref]
    python benchmarks/wgrad_dump.py --compare BASE_RUN1 BASE_RUN2 [BASE_RUN3 ...] NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of cases and writes, per case, OUTDIR/<case>.dw.npy, OUTDIR/<case>.g16.npy (the bf16
exchange twin as uint16, when the matrix is registered for one), OUTDIR/<case>.db.npy (the fused bias gradient, accumulated onto
zeros: the `single` and `batch` cases pass one), with --ref also OUTDIR/<case>.ref.npy and OUTDIR/<case>.dbref.npy (torch fp32
on the CPU), and one line "<case> <route> <sha256 dw> <sha256 g16> <sha256 dbias>" in OUTDIR/hashes.txt.  Every case runs in four
settings: overwrite / scale / registered norm accumulator + twin = 000, 111, 011, 100.  The shapes are those of
tests/test_gemm_gpu.py and tests/test_grouped_conv_gpu.py.

The second form takes two or more runs of the base build and one of the new build.  Cases whose base runs differ are the ones that
accumulate with fp32 atomics -- in all four settings of the case member, also in one on which the base runs happen to agree: for those the new dw must match
the fp32 reference of NEW_RUN at TOL_F32 (and its twin must be the rounding of its dw); every other case must be equal byte for
byte.  The bias gradient is judged on its own in the same way: equal byte for byte where the base runs agree, within TOL_DB of the
fp32 reference where they do not (every kernel adds its column sums with fp32 atomics, from two or more threads per column and from
every row split).  Exit status 1 if any case fails.
"""
import hashlib
import os
import sys
import weakref

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOL_F32 = 2e-5      # tests/test_gemm_gpu.py
TOL_DB = 1e-5       # the bias-gradient gate of tests/test_gemm_gpu.py
SETTINGS = [(0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 0)]     # overwrite, scale, registered


def route_of(geom, variant=0, msplit=0, grouped=False, v2=True):
    """Host-side mirror of wg_route (csrc/rt_wgrad.hip) for the product library's defaults."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    M = B * DH * DW
    simple = KH == 1 and KW == 1 and stride == 1 and pad == 0
    if M <= 16 and simple and SC % 4 == 0:
        return "small-M"
    if v2 and M >= 256 and N % 8 == 0 and SC % 8 == 0 and N >= 64 and SC >= 64 and variant == 0 and msplit <= 0:
        fused = KH == 3 and KW == 3 and stride == 1 and pad == 1 and SH == DH and SW == DW and DW >= 8 and N <= 128 and SC <= 128
        return "v2-fused3" if fused else "v2"
    if variant != 9 and N % 8 == 0:
        if grouped and simple and N >= 128 and SC >= 128 and M > 16 and variant == 0 and msplit <= 0:
            return "v1-dma-grouped"
        return "v1-dma"
    return "v1-reg"


def lin(M, K, N):
    return (M, 1, 1, K, 1, 1, N, 1, 1, 1, 0)


def conv(B, H, W, Ci, Co, k, s, p):
    return (B, H, W, Ci, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Co, k, k, s, p)


# name, api, [(geom, extra keyword arguments)], groups (gconv only)
CASES = [
    ("small_single", "single", [(lin(8, 256, 256), {})], 0),
    ("small_batch", "small_batch", [(lin(8, 256, 256), {}), (lin(8, 256, 256), {})], 0),
    ("v2_one_split", "single", [(lin(51200, 128, 128), {})], 0),
    ("v2_one_fused3", "single", [(conv(1, 80, 80, 128, 128, 3, 1, 1), {})], 0),
    ("v2_one_3x3", "single", [(conv(2, 40, 40, 256, 256, 3, 1, 1), {})], 0),
    # few tile tasks: the long problems are split, the 320-row one stays direct; the 3x3 / 128-channel one is the fused-tap tile
    ("batch_v2_mixed", "batch", [(lin(320, 768, 768), {}), (lin(20000, 256, 256), {}), (conv(1, 80, 80, 128, 128, 3, 1, 1), {}),
                                 (conv(2, 41, 39, 128, 128, 3, 2, 1), {})], 0),
    # second and first generation, M <= 16 and ragged members in one group
    ("batch_v1_members", "batch", [(lin(48, 256, 256), {}), (lin(200, 256, 256), {}), (lin(3520, 256, 512), {}), (lin(77, 64, 72), {}),
                                   (lin(1000, 128, 136), {}), (lin(8, 256, 256), {}), (conv(3, 9, 9, 64, 64, 3, 1, 1), {})], 0),
    ("v1_dma_v1_msplit3", "single", [(conv(2, 20, 24, 128, 128, 3, 2, 1), dict(variant=1, msplit=3))], 0),
    ("v1_dma_v2_auto", "single", [(lin(3520, 256, 2048), dict(variant=2))], 0),
    ("v1_dma_v3_auto", "single", [(lin(3520, 2048, 256), dict(variant=3))], 0),
    ("v1_dma_v5_auto", "single", [(conv(2, 20, 20, 256, 512, 1, 2, 0), dict(variant=5))], 0),
    ("v1_dma_small_tiles", "single", [(lin(200, 256, 64), {})], 0),
    ("v1_reg_variant9", "single", [(lin(320, 768, 768), dict(variant=9))], 0),
    ("v1_reg_variant9_conv", "single", [(conv(3, 21, 19, 128, 64, 3, 1, 1), dict(variant=9))], 0),
    ("v1_reg_n68", "single", [(lin(77, 64, 68), {})], 0),
    ("v1_reg_n4", "single", [(lin(48, 256, 4), {})], 0),
    ("msplit3_ws", "single", [(conv(3, 9, 9, 64, 64, 3, 1, 1), dict(msplit=3))], 0),
    ("msplit3_atomics", "single", [(conv(3, 9, 9, 64, 64, 3, 1, 1), dict(msplit=3, workspace=False))], 0),
    ("msplit1", "single", [(conv(1, 13, 17, 64, 128, 3, 2, 1), dict(msplit=1))], 0),
    # second generation: a strided gather over narrow rows (DW = 9, M = 324: every 32-row chunk wraps three or four image rows, 81 is
    # no multiple of 32 so chunks straddle images), ragged tiles with a tail chunk, an odd chunk count (65) -- alone and as one group
    # (the ragged one in the group only: builds before rt_wgrad_tile.h refuse C % 16 = 8 on the single-launch entry point)
    ("v2_strided_narrow", "single", [(conv(4, 17, 17, 64, 64, 3, 2, 1), {})], 0),
    ("v2_odd_chunks", "single", [(lin(2080, 64, 64), {})], 0),
    ("batch_v2_edges", "batch", [(conv(4, 17, 17, 64, 64, 3, 2, 1), {}), (lin(300, 72, 136), {}), (lin(2080, 64, 64), {})], 0),
    ("gconv_cg4", "gconv", [(conv(3, 7, 9, 128, 128, 3, 2, 1), dict(msplit=2))], 32),
    ("gconv_cg16", "gconv", [(conv(3, 7, 9, 1024, 1024, 3, 2, 1), {})], 64),
    ("gconv_cg64", "gconv", [(conv(3, 7, 9, 2048, 2048, 3, 2, 1), dict(msplit=3))], 32),
]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class _Owner:
    pass


def run_cases(outdir, want_ref, v2=True):
    import torch
    import torch.nn.functional as F
    from reftr_amd import hip
    os.makedirs(outdir, exist_ok=True)
    lines = []
    for ci, (name, api, members, groups) in enumerate(CASES):
        if not v2:      # the first generation stages x in 16-channel pieces
            members = [m for m in members if m[0][3] % 16 == 0]
        for ow, sc, reg in SETTINGS:
            g = torch.Generator().manual_seed(1000 + ci)
            owner = _Owner()
            slots = torch.zeros(hip.SQ_SLOTS * hip.SQ_STRIDE, device="cuda")      # one accumulator per launch group
            probs = []
            for geom, kw in members:
                B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
                cg = SC // groups if groups else SC
                x = torch.randn(B, SH, SW, SC, generator=g).bfloat16()
                dy = torch.randn(B * DH * DW, N, generator=g).bfloat16()
                dw0 = torch.randn(N, KH, KW, cg, generator=g) * 0.5
                scale = torch.rand(N, generator=g) + 0.5
                db0 = torch.zeros(N)          # (onto zeros, the two adds per column of a one-workgroup 2-threads-per-column tile commute)
                dw = dw0.cuda()
                db = db0.cuda() if api in ("single", "batch") else None
                use_scale = bool(sc) and api in ("single", "gconv") or (bool(sc) and api == "batch" and KH * KW > 1)
                twin = None
                if reg:
                    twin = torch.zeros(dw.numel(), dtype=torch.bfloat16, device="cuda")
                    hip._SQACC_MAP[dw.data_ptr()] = (weakref.ref(owner), slots)
                    hip._G16_MAP[dw.data_ptr()] = (weakref.ref(owner), twin.data_ptr())
                probs.append(dict(geom=geom, kw=kw, x=x, dy=dy, dw0=dw0, dw=dw, scale=scale if use_scale else None, twin=twin, db0=db0, db=db,
                                  xg=x.reshape(-1, SC).cuda(), dyg=dy.cuda()))
            try:
                if api == "single":
                    p = probs[0]
                    hip.conv_wgrad(p["dyg"], p["xg"], p["dw"], geom=p["geom"], overwrite=bool(ow), dbias=p["db"],
                                   scale=None if p["scale"] is None else p["scale"].cuda(), **p["kw"])
                elif api == "gconv":
                    p = probs[0]
                    hip.gconv_wgrad(p["dyg"], p["xg"], p["dw"], geom=p["geom"], groups=groups, overwrite=bool(ow),
                                    scale=None if p["scale"] is None else p["scale"].cuda(), **p["kw"])
                elif api == "small_batch":
                    b = hip.SmallWgradBatch()
                    for p in probs:
                        b.add(p["dyg"], p["xg"], p["dw"], None, overwrite=bool(ow))
                    b.run()
                else:
                    b = hip.WgradBatch(workspace_mb=256)
                    for p in probs:
                        if p["geom"][7] * p["geom"][8] > 1:
                            b.add_conv(p["dyg"], p["xg"], p["dw"], p["geom"], scale=None if p["scale"] is None else p["scale"].cuda(),
                                       overwrite=bool(ow), dbias=p["db"])
                        else:
                            b.add(p["dyg"], p["xg"], p["dw"], p["db"], overwrite=bool(ow))
                    b.run()
                torch.cuda.synchronize()
            finally:
                for p in probs:
                    hip._SQACC_MAP.pop(p["dw"].data_ptr(), None)
                    hip._G16_MAP.pop(p["dw"].data_ptr(), None)
            for mi, p in enumerate(probs):
                case = f"{name}.{mi}.ow{ow}sc{sc}reg{reg}"
                geom = p["geom"]
                route = "gconv" if api == "gconv" else "small-M-grouped" if api == "small_batch" else \
                    route_of(geom, p["kw"].get("variant", 0), p["kw"].get("msplit", 0), grouped=api == "batch", v2=v2)
                dw = p["dw"].cpu().numpy()
                np.save(os.path.join(outdir, case + ".dw.npy"), dw)
                h16 = "-"
                if p["twin"] is not None:
                    t16 = p["twin"].view(torch.int16).cpu().numpy().view(np.uint16)
                    np.save(os.path.join(outdir, case + ".g16.npy"), t16)
                    h16 = sha(t16)
                hdb = "-"
                if p["db"] is not None:
                    dbn = p["db"].cpu().numpy()
                    np.save(os.path.join(outdir, case + ".db.npy"), dbn)
                    hdb = sha(dbn)
                if want_ref:
                    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
                    xr = p["x"].float().permute(0, 3, 1, 2)
                    w = torch.zeros(N, SC // groups if groups else SC, KH, KW, requires_grad=True)
                    y = F.conv2d(xr, w, None, stride=stride, padding=pad, groups=groups or 1)
                    y.backward(p["dy"].float().reshape(B, DH, DW, N).permute(0, 3, 1, 2))
                    ref = w.grad.permute(0, 2, 3, 1)
                    if p["scale"] is not None:
                        ref = ref * p["scale"].view(-1, 1, 1, 1)
                    if not ow:
                        ref = ref + p["dw0"]
                    np.save(os.path.join(outdir, case + ".ref.npy"), ref.contiguous().numpy())
                    if p["db"] is not None:
                        np.save(os.path.join(outdir, case + ".dbref.npy"), (p["db0"] + p["dy"].float().sum(0)).numpy())
                lines.append(f"{case} {route} {sha(dw)} {h16} {hdb}")
                print(lines[-1], flush=True)
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_hashes(d):
    return {l.split()[0]: l.split() for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def compare(bases, new, table):
    import torch
    hb, hn = [read_hashes(b) for b in bases], read_hashes(new)
    h1 = hb[0]
    assert all(list(h) == list(hn) for h in hb), "the runs list different cases"
    rows, bad = [], 0
    # the four settings of a case member run the same kernels on the same split: if one of them does not reproduce itself in the base
    # runs, the member accumulates with atomics, and a setting on which the base runs happen to agree is no byte-for-byte record
    member = lambda case: case.rsplit(".", 1)[0]
    dw_atomics = {member(c) for c in h1 if not all(tuple(h[c][2:4]) == tuple(h1[c][2:4]) for h in hb)}
    db_atomics = {member(c) for c in h1 if not all(h[c][4] == h1[c][4] for h in hb)}
    for case, (_, route, d1, t1, b1) in h1.items():
        _, _, dn, tn, bn = hn[case]
        if member(case) not in dw_atomics:
            ok = (dn, tn) == (d1, t1)
            verdict = "equal" if ok else "DIFFERENT"
        else:       # fp32 atomics: the base build does not reproduce itself
            dw = np.load(os.path.join(new, case + ".dw.npy")).astype(np.float64).ravel()
            ref = np.load(os.path.join(new, case + ".ref.npy")).astype(np.float64).ravel()
            err = float(np.linalg.norm(dw - ref) / (np.linalg.norm(ref) + 1e-30))
            ok = err < TOL_F32
            if tn != "-":
                t16 = np.load(os.path.join(new, case + ".g16.npy"))
                want = torch.from_numpy(np.load(os.path.join(new, case + ".dw.npy"))).bfloat16().view(torch.int16).numpy().view(np.uint16)
                ok = ok and np.array_equal(t16.ravel(), want.ravel())
            verdict = f"atomics: rel err vs fp32 {err:.2e} " + ("ok" if ok else "FAIL")
        if b1 == "-":
            bverdict = "-"
        elif member(case) not in db_atomics:
            ok = ok and bn == b1
            bverdict = "equal" if bn == b1 else "DIFFERENT"
        else:       # the column sums meet in fp32 atomics
            db = np.load(os.path.join(new, case + ".db.npy")).astype(np.float64)
            dbref = np.load(os.path.join(new, case + ".dbref.npy")).astype(np.float64)
            berr = float(np.linalg.norm(db - dbref) / (np.linalg.norm(dbref) + 1e-30))
            ok = ok and berr < TOL_DB
            bverdict = f"atomics: rel err vs fp32 {berr:.2e} " + ("ok" if berr < TOL_DB else "FAIL")
        bad += not ok
        rows.append(f"{case:44s} {route:16s} {d1[:16]} {dn[:16]} {t1[:16]:16s} {tn[:16]:16s} {b1[:16]:16s} {bn[:16]:16s} {verdict} | dbias {bverdict}")
    text = f"{len(bases)} base runs\n{'case.member.setting':44s} {'route':16s} {'base dw':16s} {'new dw':16s} {'base g16':16s} {'new g16':16s} {'base dbias':16s} {'new dbias':16s} verdict\n" + "\n".join(rows) + \
        f"\n{len(rows)} cases, {bad} failed\n"
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
        sys.exit(compare(args[:-1], args[-1], table))
    run_cases(args[0], "--ref" in sys.argv, v2="--no-v2" not in sys.argv)
