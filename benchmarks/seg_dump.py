"""Bit-level record of the GroupNorm kernels (rt_norm.hip) and the RES-head kernels (rt_seg.hip), for comparing two builds of the library.

    python benchmarks/seg_dump.py OUTDIR
    python benchmarks/seg_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of small cases through the hip.* wrappers.  Per case it writes OUTDIR/<case>.<array>.bin (raw
fp32, bf16 as uint16) and one line "<case> <array>=<sha256> ..." in OUTDIR/hashes.txt.

The second form takes two runs of the base build and one of the new build, each from a fresh process.  Every array that the two base
runs reproduce must be byte-identical in the new run.  Arrays that the base build does not reproduce itself are listed with the largest
difference new-vs-base1 beside base1-vs-base2, and so is an array of ATOMIC_FED (summed by cross-workgroup or LDS float atomics) that
differs although the two base runs happened to agree; for them the tests' tolerances against their float references are the gate.
Exit status 1 on any other difference and on any case or array that a run lacks.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# rt_groupnorm_fwd / _bwd at B = 2: (C, G) x HW x {plain, full}.  HW = 35: fewer than 64 row blocks, two backward pixel blocks with a
# ragged second; full = pos / ypos_bf16, a row map (rows_per_img = HW + 5, row_off = 5) and dy2.
GROUPNORM = [(f"groupnorm_c{C}_hw{HW}_{'full' if full else 'plain'}", C, G, HW, full)
             for C, G in ((256, 32), (64, 8)) for HW in (35, 400) for full in (False, True)]
# rt_gn_nhwc_fwd / _bwd, the shapes of tests/test_seg_ops_gpu.py: (B, HW, C, ld, act).  C = 520: passes of 256 channels over several pixel
# blocks; C = 16: 16 pixel rows per pass; C = 128: no padding, no ReLU.
GN_NHWC = [("gn_nhwc_c520", 2, 35, 520, 576, 1), ("gn_nhwc_c16", 3, 108, 16, 64, 1), ("gn_nhwc_c128", 2, 36, 128, 128, 0),
           ("gn_nhwc_c32", 1, 400, 32, 64, 1)]
# rt_gn_nhwc_bwd with dy non-zero only where ONE thread of gn_nhwc_bstats_kernel sums (one channel per group, the pixels of one pixel
# row of the pass, one pixel block per image): every atomic target receives one non-zero add, so bstats and with it dx have one value
# and dx is compared byte for byte.  (Not under the "gn_nhwc" prefix of ATOMIC_FED on purpose.)
GN_ONE_THREAD = [("gn1thread_c32", 2, 100, 32, 64, 1), ("gn1thread_c128", 2, 30, 128, 128, 0)]
UPSAMPLE = [("upsample_2x", 2, 5, 7, 10, 14, 128, 128), ("upsample_ragged", 1, 13, 9, 25, 18, 32, 64), ("upsample_c64", 2, 4, 4, 8, 8, 64, 64)]
ATTN_MAP = [("attn_map_small", 2, 5, 7, 3), ("attn_map_400", 3, 20, 20, 40)]
CONCAT = [("seg_concat_dense", True), ("seg_concat_mapped", False)]
MASK_LOSS = [("mask_loss_4x", 2, 24, 32, 96, 128), ("mask_loss_ragged", 3, 10, 13, 37, 50)]
# rt_cem_fwd / _bwd at B = 2, E = 256, ld = 64.  HW = 35: most of the 1024 threads hold -inf; HW = 1100: a thread takes a second pixel.
CEM = [("cem_hw35", 35), ("cem_hw1100", 1100)]


# Arrays summed by cross-workgroup or LDS float atomics, by case prefix: gn_bwd_stats_kernel / gn_nhwc_bstats_kernel add bstats (which
# every dx reads), dgamma and dbeta; cem_fwd_kernel / cem_bwd_kernel add the loss and the parameter gradients.
ATOMIC_FED = {"groupnorm": ("dx_f32", "dx_bf16", "dgamma", "dbeta"), "gn_nhwc": ("dx", "dgamma", "dbeta"), "cem": ("loss", "dw3", "db3", "dw2")}


def atomic_fed(case, key):
    return any(case.startswith(p) and key in keys for p, keys in ATOMIC_FED.items())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cases():
    """Yields (case name, {array name: tensor}); needs a GPU."""
    import torch
    from reftr_amd import hip

    def gen(seed):
        return torch.Generator().manual_seed(seed)

    def rn(g, *shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda()

    for ci, (name, C, G, HW, full) in enumerate(GROUPNORM):
        g, B = gen(4000 + ci), 2
        S, off = (HW + 5, 5) if full else (HW, 0)
        x = rn(g, B, HW, C); gam = (torch.rand(C, generator=g) + 0.5).cuda(); bet = rn(g, C, scale=0.1)
        pos, dy, dy2 = rn(g, B * S, C), rn(g, B * S, C), rn(g, B * S, C)
        yf = torch.zeros(B * S, C, device="cuda"); yb = torch.zeros(B * S, C, device="cuda", dtype=torch.bfloat16); ypb = torch.zeros_like(yb)
        stats = hip.groupnorm_fwd(x, gam, bet, G, 1e-5, y_f32=yf, y_bf16=yb, pos=pos if full else None, ypos_bf16=ypb if full else None,
                                  rows_per_img=S, row_off=off)
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dxf, dxb = hip.groupnorm_bwd(dy, x, gam, stats, dg, db, G, 1e-5, dy2=dy2 if full else None, rows_per_img=S, row_off=off, want_f32=True)
        yield name, dict(y_f32=yf, y_bf16=yb, ypos_bf16=ypb, stats=stats, dx_f32=dxf, dx_bf16=dxb, dgamma=dg, dbeta=db)

    for ci, (name, B, HW, C, ld, act) in enumerate(GN_NHWC):
        g = gen(4100 + ci)
        x = torch.full((B * HW, ld), 7.0); x[:, :C] = torch.randn(B * HW, C, generator=g); x = x.cuda()        # non-zero padding
        gam = (torch.rand(C, generator=g) + 0.5).cuda(); bet = rn(g, C, scale=0.2)
        dy = torch.zeros(B * HW, ld); dy[:, :C] = torch.randn(B * HW, C, generator=g); dy = dy.cuda()
        y, stats = hip.gn_nhwc_fwd(x, gam, bet, B, HW, C, 8, ldy=ld, act=act)
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dx = hip.gn_nhwc_bwd(dy, x, gam, bet, stats, dg, db, B, HW, C, 8, lddx=ld, act=act)
        yield name, dict(y=y, stats=stats, dx=dx, dgamma=dg, dbeta=db)

    for ci, (name, B, HW, C, ld, act) in enumerate(GN_ONE_THREAD):
        g = gen(4150 + ci)
        x = torch.full((B * HW, ld), 7.0); x[:, :C] = torch.randn(B * HW, C, generator=g); x = x.cuda()
        gam = (torch.rand(C, generator=g) + 0.5).cuda(); bet = rn(g, C, scale=0.2)
        rows = 256 // C                                                    # pixel rows per pass (C divides 256)
        dy = torch.zeros(B * HW, ld)
        dy.view(B, HW, ld)[:, ::rows, 0:C:C // 8] = torch.randn(B, len(range(0, HW, rows)), 8, generator=g)
        y, stats = hip.gn_nhwc_fwd(x, gam, bet, B, HW, C, 8, ldy=ld, act=act)
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dx = hip.gn_nhwc_bwd(dy.cuda(), x, gam, bet, stats, dg, db, B, HW, C, 8, lddx=ld, act=act)
        yield name, dict(dx=dx, dgamma=dg, dbeta=db)

    for ci, (name, B, h, w, H, W, C, ld) in enumerate(UPSAMPLE):
        g = gen(4200 + ci)
        a = torch.zeros(B * h * w, ld); a[:, :C] = torch.randn(B * h * w, C, generator=g)
        fpn = rn(g, B * H * W, C)
        dy = torch.zeros(B * H * W, ld); dy[:, :C] = torch.randn(B * H * W, C, generator=g)
        out = hip.upsample_add(fpn, a.bfloat16().cuda(), B, H, W, h, w, C, ldo=ld)
        da, dyb = hip.upsample_add_bwd(dy.cuda(), B, H, W, h, w, C, ldda=ld, lddyb=ld)
        yield name, dict(out=out, da=da, dyb=dyb)

    for ci, (name, B, h, w, L) in enumerate(ATTN_MAP):
        g, E, nh = gen(4300 + ci), 256, 8
        HW, S = h * w, L + h * w
        q, k = rn(g, B, E), rn(g, B * S, E, scale=0.3)
        mask = torch.zeros(B, h, w, dtype=torch.uint8); mask[1, :, w - 2:] = 1; mask[1, h - 1:, :] = 1       # image 1 partly masked
        concat = torch.full((B * HW, 576), 3.0, dtype=torch.bfloat16, device="cuda")
        P = hip.attn_map_fwd(q, k, mask.reshape(B, HW).cuda(), B, HW, E, nh, S, L, concat=concat, concat_col=512)
        dcon = torch.zeros(B * HW, 576); dcon[:, 512:520] = torch.randn(B * HW, nh, generator=g)
        dq, dk = hip.attn_map_bwd(q, k, P, dcon.cuda(), B, HW, E, nh, S, L, 512)
        yield name, dict(P=P, concat=concat, dq=dq, dk=dk)

    for ci, (name, dense) in enumerate(CONCAT):
        g, B, HW, E, nh, L = gen(4400 + ci), 2, 35, 256, 8, 5
        src = rn(g, B * HW if dense else B * (L + HW), E); mem = rn(g, B * (L + HW), E)
        out = torch.full((B * HW, 576), 9.0, dtype=torch.bfloat16, device="cuda")
        hip.seg_concat(src, mem, out, B, HW, E, nh, L + HW, L, src_dense=dense)
        yield name, dict(out=out)

    for ci, (name, B, h, w, Ht, Wt) in enumerate(MASK_LOSS):
        g = gen(4500 + ci)
        pp = torch.zeros(B * h * w, 4); pp[:, 0] = torch.randn(B * h * w, generator=g) * 2; pp = pp.cuda()
        tgt = (torch.rand(B, Ht, Wt, generator=g) > 0.6).to(torch.uint8).cuda()
        losses, sums = hip.mask_loss(pp, tgt, B, h, w, Ht, Wt, 4, float(B))
        dpred = torch.zeros(B * h * w, 64, device="cuda")
        hip.mask_loss(pp, tgt, B, h, w, Ht, Wt, 4, float(B), sums=sums, dpred=dpred, g_focal=torch.tensor([0.7], device="cuda"),
                      g_dice=torch.tensor([1.3], device="cuda"))
        yield name, dict(losses=losses, sums=sums, dpred=dpred)

    for ci, (name, HW) in enumerate(CEM):
        g, B, E, ld = gen(4600 + ci), 2, 256, 64
        hs = rn(g, B, E).bfloat16(); w3 = rn(g, 16, E, scale=0.1); b3 = rn(g, 16, scale=0.1); w2 = rn(g, 16, scale=0.5); b2 = rn(g, 1, scale=0.1)
        res = torch.zeros(B * HW, ld); res[:, :16] = torch.randn(B * HW, 16, generator=g).relu(); res = res.bfloat16().cuda()
        loss, saved = hip.cem_fwd(hs, w3, b3, res, w2, b2, B, HW)
        dres = rn(g, B * HW, ld, scale=0.01)
        dw3, db3, dw2 = torch.zeros(16, E, device="cuda"), torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
        dhs = hip.cem_bwd(hs, w3, b3, res, w2, b2, saved, torch.tensor([0.8], device="cuda"), dres, dw3, db3, dw2, B, HW)
        yield name, dict(loss=loss, u=saved[0], energy=saved[1], stats=saved[2], dres=dres, dhs=dhs, dw3=dw3, db3=db3, dw2=dw2)


def case_names():
    return [c[0] for group in (GROUPNORM, GN_NHWC, GN_ONE_THREAD, UPSAMPLE, ATTN_MAP, CONCAT, MASK_LOSS, CEM) for c in group]


def run_all(outdir):
    import torch
    os.makedirs(outdir, exist_ok=True)
    lines = []
    for name, arrays in cases():
        torch.cuda.synchronize()
        hs = []
        for key, t in arrays.items():
            a = t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()
            a.tofile(os.path.join(outdir, f"{name}.{key}.bin"))
            hs.append(f"{key}={sha(a)}:{'u2' if a.dtype == np.uint16 else 'f4'}")
        lines.append(name + " " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def read_hashes(d):
    return {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def max_diff(d1, d2, case, key, kind):
    """Largest |a - b| of one array of two runs; bf16 (stored as uint16) is widened to fp32 first."""
    def load(d):
        a = np.fromfile(os.path.join(d, f"{case}.{key}.bin"), dtype=np.uint16 if kind == "u2" else np.float32)
        return (a.astype(np.uint32) << 16).view(np.float32) if kind == "u2" else a
    a, b = load(d1), load(d2)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.shape == b.shape else float("inf")


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    want = case_names()
    rows, bad, n_arrays, n_unstable = [], 0, 0, 0
    for case in want:
        lacking = [n for n, h in (("base1", h1), ("base2", h2), ("new", hn)) if case not in h or set(h[case]) != set(h1.get(case, {})) or not h[case]]
        if lacking:
            bad += 1
            rows.append(f"{case:28s} MISSING or incomplete in " + " ".join(lacking))
            continue
        for key, hv in h1[case].items():
            n_arrays += 1
            digest, kind = hv.split(":")
            stable, same = h2[case][key] == hv, hn[case][key] == hv
            n_unstable += not stable
            if stable and same:
                verdict = "equal"
            elif stable and not atomic_fed(case, key):
                verdict = "DIFFERENT"
                bad += 1
            else:           # summed by float atomics: the order of the adds is the hardware's, and two equal base runs do not fix it
                dn, db = max_diff(new, base1, case, key, kind), max_diff(base1, base2, case, key, kind)
                verdict = "%s: max |new - base1| %.3e, max |base1 - base2| %.3e%s" % (
                    "float atomics, base runs equal" if stable else "base runs differ", dn, db,
                    "   <-- LOOK: more than 10 x the base runs' own difference" if stable or dn > 10 * db else "")
            rows.append(f"{case:28s} {key:10s} {digest[:8]}/{hn[case][key][:8]} {verdict}")
    extra = sorted((set(h1) | set(h2) | set(hn)) - set(want))
    bad += len(extra)
    text = "sha256 (first 8 digits) of every array, base build / new build\n" + \
        f"{'case':28s} {'array':10s} {'base/new':17s} verdict\n" + "\n".join(rows) + \
        "".join(f"\n{c}: not a case of this tool" for c in extra) + \
        f"\n{len(want)} cases, {n_arrays} arrays, {n_unstable} not reproduced by the base build itself, {bad} failed\n"
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
