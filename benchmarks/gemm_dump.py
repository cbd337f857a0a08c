"""Bit-level record of every rt_conv_gemm route, for comparing two builds of the library.

    python benchmarks/gemm_dump.py OUTDIR
    python benchmarks/gemm_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of cases in every setting of SETTINGS, one child process per setting, one after the other
(the lab switches are read once per process and need the lab library, REFTR_LAB=1).  Per setting and case it writes
OUTDIR/<setting>.<case>.{f32,bf16}.bin (raw fp32 / bf16 as uint16; every output of a multi-product case concatenated) and one line
"<setting>.<case> <sha256 f32> <sha256 bf16>" in OUTDIR/hashes.txt.  A child that fails ends the run.

The second form takes two runs of the base build and one of the new build.  The GEMM kernels use no atomics: the two base runs must
agree, and every case of the new run must equal them byte for byte.  Exit status 1 otherwise.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCT_HINTS = [0, 21, 31, 33, 51, 233, 252, 262, 281, 285]
GATHER_HINTS = [0, 21, 31, 33, 51, 233, 252]                       # the product variants that are not dense-only
LAB_HINTS = [1, 2, 3, 11, 12, 13, 22, 32, 52, 53, 54, 61, 62, 63, 211, 221, 231, 251, 261, 81, 282, 283, 284, 286, 287, 288, 234, 236,
             351, 321, 323, 331, 352, 322, 332, 501]
SWITCHES = ["REFTR_EARLY", "REFTR_EPI", "REFTR_EPI_PREFETCH", "REFTR_XCD", "REFTR_S2PARITY"]
# setting -> (environment of its process, case list)
SETTINGS = [("product", {}, "product"), ("lab", {"REFTR_LAB": "1"}, "lab")] + \
           [("lab_" + s[6:].lower() + "0", {"REFTR_LAB": "1", s: "0"}, "switch") for s in SWITCHES]
# B, H, W, Cin, Cout, k, stride, pad, dil
CONVS = {"c3s1": (2, 20, 20, 64, 64, 3, 1, 1, 1), "c3s2": (2, 20, 24, 128, 128, 3, 2, 1, 1), "c3s2odd": (1, 13, 17, 64, 128, 3, 2, 1, 1),
         "c3d2": (1, 13, 9, 64, 128, 3, 1, 2, 2)}
EPI_FIELDS = ["relu", "gelu", "tanh", "res", "res_first", "gate", "preact", "dtanh", "drop", "drop4", "out_preact", "acc2"]


def cases(kind):
    """(name, function of (hip, torch generator) -> list of output tensors)"""
    out = []
    if kind == "product":
        for K in (256, 512, 2048):                                   # skinny kernel: 2, 4 and 8 k-steps per wave in flight
            out.append((f"skinny_k{K}", lambda hip, g, K=K: dense(hip, g, 8, K, 256, 0, "res")))
        for h in PRODUCT_HINTS:
            out.append((f"dense_h{h}", lambda hip, g, h=h: dense(hip, g, 333, 192, 264, h)))
        for name in ("c3s1", "c3s2", "c3s2odd"):
            for h in GATHER_HINTS:
                out.append((f"{name}_h{h}", lambda hip, g, name=name, h=h: conv(hip, g, CONVS[name], h)))
        out.append(("c3d2_h0", lambda hip, g: conv(hip, g, CONVS["c3d2"], 0)))
        out.append(("grouped3", lambda hip, g: grouped(hip, g, [(3520, 256, 512), (333, 512, 264), (100, 768, 64)])))
        out.append(("grouped_fallback", lambda hip, g: grouped(hip, g, [(8, 256, 256), (512, 2048, 256), (333, 192, 264)])))
        for M, N in ((333, 192), (333, 196), (12, 192)):             # 8-wide, 4-wide, skinny (prefetched) epilogue
            for f in EPI_FIELDS:
                out.append((f"epi_{M}x{N}_{f}", lambda hip, g, M=M, N=N, f=f: dense(hip, g, M, 128, N, 0, f)))
    elif kind == "lab":
        for h in LAB_HINTS:
            out.append((f"dense_h{h}", lambda hip, g, h=h: dense(hip, g, 333, 256 if h == 501 else 192, 264, h)))
        for h in (11, 22, 32, 52, 63, 211, 231, 251, 351, 322, 332):
            out.append((f"c3s2_h{h}", lambda hip, g, h=h: conv(hip, g, CONVS["c3s2"], h)))
        out.append(("epi_h501_res", lambda hip, g: dense(hip, g, 333, 128, 192, 501, "res")))
        out.append(("epi_h352_gate", lambda hip, g: dense(hip, g, 333, 128, 192, 352, "gate")))
    else:
        out.append(("dense_h31_res", lambda hip, g: dense(hip, g, 333, 192, 264, 31, "res")))
        out.append(("dense_h0_gate", lambda hip, g: dense(hip, g, 3520, 256, 512, 0, "gate")))
        out.append(("c3s2_h0", lambda hip, g: conv(hip, g, CONVS["c3s2"], 0)))
    return out


def dense(hip, g, M, K, N, hint, field=None):
    import torch
    r = lambda *s: torch.randn(*s, generator=g)
    x, w, b = r(M, K).bfloat16().cuda(), (r(N, K) / K ** 0.5).bfloat16().cuda(), r(N).cuda()
    rf, rb, t = r(M, N).cuda(), r(M, N).bfloat16().cuda(), r(M, N).bfloat16().cuda()
    kw = {"relu": dict(act=hip.ACT_RELU), "gelu": dict(act=hip.ACT_GELU), "tanh": dict(act=hip.ACT_TANH),
          "res": dict(res_f32=rf, res_bf16=rb), "res_first": dict(res_f32=rf, res_bf16=rb, res_first=True, act=hip.ACT_RELU),
          "gate": dict(gate=t, gate_scale=1.25, res_bf16=rb), "preact": dict(preact=t), "dtanh": dict(dtanh=t),
          "drop": dict(drop_p=0.1, drop_seed=1234), "drop4": dict(drop_p=0.1, drop_seed=1234, drop_shift=2),
          "out_preact": dict(act=hip.ACT_RELU, out_preact=True), "acc2": dict(acc2_f32=rf), None: {}}[field]
    outs = hip.linear(x, w, bias=b, out_bf16=True, out_f32=True, tile_hint=hint, **kw)
    return list(outs) + ([rf] if field == "acc2" else [])


def conv(hip, g, geom, hint):
    """forward gather and transposed (backward-data) gather of one convolution"""
    import torch
    B, H, W, Ci, Co, k, s, p, dil = geom
    Ho, Wo = (H + 2 * p - dil * (k - 1) - 1) // s + 1, (W + 2 * p - dil * (k - 1) - 1) // s + 1
    r = lambda *sh: torch.randn(*sh, generator=g)
    x, w, b = r(B, H, W, Ci).bfloat16().cuda(), (r(Co, k, k, Ci) / (Ci * k * k) ** 0.5).bfloat16().cuda(), r(Co).cuda()
    dy, wt = r(B, Ho, Wo, Co).bfloat16().cuda(), (r(Ci, k, k, Co) / (Co * k * k) ** 0.5).bfloat16().cuda()
    f = hip.conv_gemm(x, w, geom=(B, H, W, Ci, Ho, Wo, Co, k, k, s, p), bias=b, out_bf16=True, out_f32=True, tile_hint=hint, dil=dil)
    t = hip.conv_gemm(dy, wt, geom=(B, Ho, Wo, Co, H, W, Ci, k, k, s, p), transposed=True, out_bf16=True, out_f32=True, tile_hint=hint, dil=dil)
    return list(f) + list(t)


def grouped(hip, g, shapes):
    import torch
    grp, outs = hip.GemmGroup(), []
    for M, K, N in shapes:
        x = torch.randn(M, K, generator=g).bfloat16().cuda(); w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().cuda()
        outs += list(hip.linear(x, w, bias=torch.randn(N, generator=g).cuda(), out_bf16=True, out_f32=True, group=grp))
    grp.run()
    return outs


def run_setting(setting, outdir):
    import torch
    from reftr_amd import hip
    hip.set_seed_dev(None)
    kind = {s: k for s, _, k in SETTINGS}[setting]
    lines = []
    for ci, (name, fn) in enumerate(cases(kind)):
        outs = fn(hip, torch.Generator().manual_seed(3000 + ci))
        torch.cuda.synchronize()
        hs = []
        for key, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            parts = [(t.view(torch.int16) if dt == torch.bfloat16 else t).cpu().numpy().ravel() for t in outs if t is not None and t.dtype == dt]
            a = np.concatenate(parts)
            a = a.view(np.uint16) if a.dtype == np.int16 else a
            a.tofile(os.path.join(outdir, f"{setting}.{name}.{key}.bin"))
            hs.append(hashlib.sha256(a.tobytes()).hexdigest())
        lines.append(f"{setting}.{name} " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, f"hashes.{setting}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def run_all(outdir):
    os.makedirs(outdir, exist_ok=True)
    text = ""
    for setting, extra, _ in SETTINGS:
        env = dict(os.environ)
        for k in ["REFTR_LAB"] + SWITCHES:
            env.pop(k, None)
        env.update(extra)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, outdir], check=True, env=env, timeout=300)
        text += open(os.path.join(outdir, f"hashes.{setting}.txt")).read()
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write(text)


def read_hashes(d):
    return {l.split()[0]: l.split()[1:] for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    assert list(h1) == list(h2) == list(hn), "the three runs list different cases"
    rows, bad, unstable = [], 0, 0
    for case, hs in h1.items():
        stable, same = h2[case] == hs, hn[case] == hs
        verdict = "equal" if stable and same else "BASE RUNS DIFFER" if not stable else "DIFFERENT"
        bad += not (stable and same)
        unstable += not stable
        rows.append(f"{case:34s} " + " ".join(f"{a[:10]}/{b[:10]}" for a, b in zip(hs, hn[case])) + f" {verdict}")
    text = f"{'setting.case':34s} {'f32 base/new':21s} {'bf16 base/new':21s} verdict\n" + "\n".join(rows) + \
        f"\n{len(rows)} cases, {unstable} not reproduced by the base build itself, {bad} failed\n"
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
    if "--child" in sys.argv:
        run_setting(args[0], args[1])
    else:
        run_all(args[0])
