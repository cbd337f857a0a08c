"""Bit-level record of every attention route, for comparing two builds of the library.

    python benchmarks/attn_dump.py OUTDIR
    python benchmarks/attn_dump.py --compare BASE_RUN1 BASE_RUN2 NEW_RUN [--table FILE]

The first form runs a fixed, seeded list of cases in every setting of SETTINGS, one child process per setting, one after the other
(the library reads REFTR_ATTN_CHUNK and the lab switches once per process; the lab switches need the lab library, REFTR_LAB=1).  Per
setting and case it writes OUTDIR/<setting>.<case>.{o,lse,dq,dk,dv}.bin (raw bf16 as uint16, lse as float32) and one line
"<setting>.<case> <route> <sha256 o> <lse> <dq> <dk> <dv>" in OUTDIR/hashes.txt (route: the intended one, from route_of).  A child that fails ends the run.

The second form takes two runs of the base build and one of the new build.  Attention uses no atomics: the two base runs must agree,
and every case of the new run must equal them byte for byte (bytes, not values: a fully masked row is NaN).  Exit status 1 otherwise.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# setting -> environment of its process
SETTINGS = [
    ("product", {}),
    ("chunk64", {"REFTR_ATTN_CHUNK": "64"}),
    ("chunk224", {"REFTR_ATTN_CHUNK": "224"}),
    ("lab_nw4", {"REFTR_LAB": "1", "REFTR_ATTN_NW": "4"}),
    ("lab_nw16", {"REFTR_LAB": "1", "REFTR_ATTN_NW": "16"}),
    ("lab_reg0", {"REFTR_LAB": "1", "REFTR_ATTN_REG": "0"}),
    ("lab_unfused", {"REFTR_LAB": "1", "REFTR_ATTN_BWD_FUSED": "0"}),
    ("lab_q1off", {"REFTR_LAB": "1", "REFTR_ATTN_Q1": "0"}),
]
# name, (B, H, Sq, Sk, dh), drop_p, mask: None | "tail" (masked tail + scattered keys) | "row" (batch 0 fully masked: NaN)
CASES = [
    ("q1_drop", (2, 2, 1, 440, 32), 0.1, "tail"),
    ("q1_plain", (1, 2, 1, 700, 32), 0.0, None),
    ("reg8_dh32", (2, 2, 100, 128, 32), 0.1, "tail"),
    ("reg8_dh64", (2, 2, 40, 40, 64), 0.0, None),
    ("reg28_dh32", (2, 2, 440, 440, 32), 0.1, "tail"),
    ("reg28_dh64", (1, 2, 130, 440, 64), 0.0, "tail"),
    ("twopass_dh32", (1, 2, 130, 715, 32), 0.1, "tail"),
    ("twopass_dh64", (1, 2, 70, 470, 64), 0.1, None),
    ("long_sk_dh32", (1, 2, 70, 1000, 32), 0.1, "tail"),
    ("long_sq_dh32", (1, 2, 900, 33, 32), 0.1, None),
    ("long_dh64", (1, 2, 200, 600, 64), 0.0, "tail"),
    ("masked_row", (2, 2, 50, 100, 32), 0.0, "row"),
]
ARRAYS = ("o", "lse", "dq", "dk", "dv")


def route_of(setting, shape):
    """Host-side mirror of the dispatch in rt_attn_fwd / rt_attn_bwd (csrc/rt_attention.hip): forward / backward kernel."""
    B, H, Sq, Sk, dh = shape
    env = dict(SETTINGS)[setting]
    if env.get("REFTR_ATTN_Q1", "1") != "0" and Sq == 1 and dh == 32 and Sk <= 768:
        return "q1/q1"
    smem = lambda n: 2 * ((n + 31) & ~31) * (dh * 2 + 32) + 8 * ((n + 31) & ~31)
    forced = "REFTR_ATTN_CHUNK" in env
    fwd_long, bwd_long = forced or smem(Sk) > 160 * 1024, forced or smem(Sk) > 160 * 1024 or smem(Sq) > 160 * 1024
    nw = int(env.get("REFTR_ATTN_NW", "8"))
    tiles = ((Sk + 31) & ~31) >> 4
    if fwd_long:
        fwd = "long"
    elif env.get("REFTR_ATTN_REG", "1") != "0" and nw == 8 and tiles <= 28:
        fwd = "reg8" if tiles <= 8 else "reg28"
    else:
        fwd = f"twopass-nw{nw}"
    bwd = "long" if bwd_long else "fused" if env.get("REFTR_ATTN_BWD_FUSED", "1") != "0" and nw == 8 else f"dq+dkv-nw{nw}"
    return fwd + "/" + bwd


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_setting(setting, outdir):
    import torch
    from reftr_amd import hip
    hip.set_seed_dev(None)
    lines = []
    for ci, (name, (B, H, Sq, Sk, dh), drop_p, mask) in enumerate(CASES):
        E = H * dh
        g = torch.Generator().manual_seed(2000 + ci)
        q, k, v, do = (torch.randn(B * n, E, generator=g).bfloat16().cuda() for n in (Sq, Sk, Sk, Sq))
        kpm = None
        if mask:
            kpm = torch.zeros(B, Sk, dtype=torch.uint8)
            kpm[B - 1, Sk - max(1, Sk // 7):] = 1
            kpm[B - 1, 1::37] = 1
            if mask == "row":
                kpm[0, :] = 1
            kpm = kpm.cuda()
        kw = dict(B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, scale=dh ** -0.5, drop_p=drop_p, drop_seed=77 + ci)
        o, lse = hip.attn_fwd(q, k, v, kpm, **kw)
        dq, dk, dv = hip.attn_bwd(q, k, v, o, do, lse, kpm, **kw)
        torch.cuda.synchronize()
        hs = []
        for key, t in zip(ARRAYS, (o, lse, dq, dk, dv)):
            a = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
            a = a.view(np.uint16) if a.dtype == np.int16 else a
            a.tofile(os.path.join(outdir, f"{setting}.{name}.{key}.bin"))
            hs.append(sha(a))
        lines.append(f"{setting}.{name} {route_of(setting, (B, H, Sq, Sk, dh))} " + " ".join(hs))
        print(lines[-1], flush=True)
    with open(os.path.join(outdir, f"hashes.{setting}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def run_all(outdir):
    os.makedirs(outdir, exist_ok=True)
    text = ""
    for setting, extra in SETTINGS:
        env = dict(os.environ)
        for k in ("REFTR_LAB", "REFTR_ATTN_CHUNK", "REFTR_ATTN_NW", "REFTR_ATTN_REG", "REFTR_ATTN_BWD_FUSED", "REFTR_ATTN_Q1"):
            env.pop(k, None)
        env.update(extra)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, outdir], check=True, env=env, timeout=600)
        text += open(os.path.join(outdir, f"hashes.{setting}.txt")).read()
    with open(os.path.join(outdir, "hashes.txt"), "w") as f:
        f.write(text)


def read_hashes(d):
    return {l.split()[0]: l.split()[1:] for l in open(os.path.join(d, "hashes.txt")) if l.strip()}


def compare(base1, base2, new, table):
    h1, h2, hn = read_hashes(base1), read_hashes(base2), read_hashes(new)
    assert list(h1) == list(h2) == list(hn), "the three runs list different cases"
    rows, bad, unstable = [], 0, 0
    for case, (route, *hs) in h1.items():
        stable = h2[case][1:] == hs
        same = [a == b for a, b in zip(hs, hn[case][1:])]
        ok = stable and all(same)
        verdict = "equal" if ok else "BASE RUNS DIFFER" if not stable else "DIFFERENT: " + " ".join(k for k, s in zip(ARRAYS, same) if not s)
        bad += not ok
        unstable += not stable
        rows.append(f"{case:28s} {route:22s} " + " ".join(f"{a[:10]}/{b[:10]}" for a, b in zip(hs, hn[case][1:])) + f" {verdict}")
    text = "route: the kernels the host dispatch is meant to choose (route_of, a mirror of rt_attn_fwd / rt_attn_bwd; not reported by the library)\n" + \
        f"{'setting.case':28s} {'route fwd/bwd':22s} " + " ".join(f"{k + ' base/new':21s}" for k in ARRAYS) + " verdict\n" + "\n".join(rows) + \
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
