"""GPU: the tile kernels behind rt_conv_gemm / rt_conv_gemm_grouped and the weight-gradient kernels behind rt_conv_wgrad /
rt_conv_wgrad_grouped, element by element against float64 (oracle/gemm_ref.py, pinned to autograd and its bounds proven usable on a
CPU emulation by tests/test_gemm_ref_cpu.py, whose cases, inputs and check functions this file runs on the kernels).  The product
library only; the lab-only hints stay with tests/test_gemm_gpu.py.

Every output is a view of a larger buffer with GUARD rows before and after it, everything pre-filled with PATTERN (a finite number):
after each call the guards hold the pattern bit for bit and no owned element does.

  tier 1, exact   integer operands (x, w, dy in -3 .. 3; bias, residuals, acc2, the preloaded dw integers; scale and gate_scale powers
                  of two; drop_p = 0.5): every partial sum is an integer below 2^24, so out_f32, out_bf16, out_preact, acc2_f32, dw,
                  dbias and the bf16 twin have ONE legal value per element whatever the summation order, split count or atomics;
                  one-hot probes (one source pixel per image swept over corners, edges and interior; one dy row) turn a wrong tap,
                  pad, stride, dilation or tile offset into whole wrong elements
  tier 2, rounding  bf16-rounded randn operands, an ill-conditioned set whose products cancel to ~2^-6 of sum |x w|, and operands
                  scaled by 16, at the bounds of oracle/gemm_ref.py (u = 2^-23): fp32 (K + 2) u (|x| |w|^T + |bias| + |res|) carried
                  through the epilogue, weight gradients (M + S + 2) u |scale| sum |dy x| + u |dw before|, bf16 + 2^-8 |ref|,
                  sqacc (N K + 256 + 4) u sum (after^2 + before^2); GELU / tanh / gelu' add the error of the fp32 expressions
                  measured on the CPU (gelu 0.86 u |x|, tanh 0.53 u |tanh x|, gelu' 0.55 u (1 + |x|)) times 2 for the device's
                  math library

Worst error / bound per tensor and path over all cases and operand sets of tier 2, measured on the MI355X (every test prints its
own; tier 1 is bit-exact on every path, the one-hot probes included).  bf16 stores sit just under 1: half an ulp is the rounding
every one of them makes; the fp32 bounds are worst-case bounds over every summation order and the kernels use a few per cent of them
-- the sharp check of the fp32 values is tier 1:
  tile forms (hints 21, 31, 33, 51, 233, 252, 262, 281, 285)   out_f32 0.01, out_bf16 0.99
  skinny route / first tile route (hint 0, M = 16 / 17)         out_f32 0.01, out_bf16 0.95
  GemmGroup of three                                            out_f32 0.00, out_bf16 0.96
  gathers, forward and transposed (21, 31, 33, 51, 233, 252)    out_f32 0.01, out_bf16 0.98
  epilogue combinations (hint 0 and the nine forms)             out_f32 0.08, out_bf16 0.99, out_preact 0.98, acc2 0.01
                                                                (out_f32's worst are the GELU / tanh / gelu' combinations: the
                                                                device's erff, tanhf, __expf inside twice the host's error)
  first-generation weight gradients, six (N, SC)                dw 0.01, dbias 0.00, g16 0.99, sq 0.00
  ... gathers                                                   dw 0.00, dbias 0.00, g16 0.97, sq 0.00
  second generation, alone and grouped                          dw 0.01, dbias 0.00, g16 0.98, sq 0.00
Every guard intact, no poison left in owned memory.  The whole file (48 tests, about 2400 launches) takes 11 - 13 s on the MI355X.

Scratch mutations (one line each, values only, on a copy, not committed), which tests of this file noticed them and whether
tests/test_gemm_gpu.py (its lab-library child included) did:
  transposed stride-2 gather: the parity class's `(ny_ | nx_) >= 0` made `> 0`     gathers and one-hot source pixels on all 6 hints;
      (rt_gemm_dma.h; the divisibility test of the product path)                    test_gemm_gpu.py: 22 tests (conv_dma_variants, conv_fwd_dgrad_wgrad)
  8-wide epilogue: the prefetched gate taken from the piece before                  epilogue combinations on every hint that prefetches (0, 21, 31, 33, 233,
      (epi_prefetch, rt_gemm_common.h)                                              252, 281, 285; 51 and 262 hold no prefetched pieces); test_gemm_gpu.py:
                                                                                    test_linear_epilogue on 9 hints
  res_first ignored when only the bf16 store is on                                  epilogue combinations on all 10 hints (tier 1, "out_bf16 alone":
      (`if (p.res_first && p.out_f32) add_res()`)                                   489 of 1088 elements of the first case); test_gemm_gpu.py: NOTHING
  a weight-gradient split that drops its last chunk when it is ragged               all six first-generation (N, SC), the gathers (since their cases reach a
      (wg_chunks, rt_wgrad_tile.h)                                                  ragged last split), the second generation at all four operand sets;
                                                                                    test_gemm_gpu.py: 52 tests
  kh and kw exchanged under dilation in the forward gather                          gathers and one-hot source pixels on all 6 hints; test_gemm_gpu.py:
                                                                                    test_dilated_conv_fwd_dgrad_wgrad (4)
  bf16 stores truncated instead of rounded (to_bf16 of the epilogue)                35 tests: every rt_conv_gemm test of this file; test_gemm_gpu.py: 43 tests
  the bf16 twin written before dw is accumulated (rt_wg_commit)                     second generation at all four operand sets and its one-hot dy rows;
                                                                                    test_gemm_gpu.py: NOTHING (no test of it reads the twin or sqacc)
"""
import weakref

import pytest
import torch

from oracle import gemm_ref as G
from test_gemm_ref_cpu import (KINDS, check_gemm, check_wgrad, epilogue_shape, epilogue_specs, gather_specs, gemm_spec, linear_geom, tile_specs,
                               w2_spec, wgrad_first_gen_specs, wgrad_gather_specs, wgrad_spec)
from test_region_fp64_gpu import Worst, c64

pytestmark = pytest.mark.gpu

GUARD = 2                                # rows before and after every [M, N] output
GUARD_FLAT = 64                          # elements before and after a flat one (dw, dbias, the twin)
PATTERN = {torch.bfloat16: 0x5A5B, torch.float32: 0x5A5B5A5B}       # 1.5e16 in both formats
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
EPI_KINDS = ("ints", "randn", "cancel")


# ------------------------------------------------------------------------------------------------ poisoned, guarded buffers
class Guarded:
    """`numel` elements of `dtype` (rows x cols when 2-D) inside a larger buffer; everything holds PATTERN, then `init` if given"""

    def __init__(self, shape, dtype, init=None, guard=None):
        cols = shape[-1] if len(shape) == 2 else 1
        n = shape[0] * cols if len(shape) == 2 else shape[0]
        self.g = (GUARD * cols if len(shape) == 2 else GUARD_FLAT) if guard is None else guard
        self.buf = torch.empty(n + 2 * self.g, dtype=dtype, device="cuda")
        self.buf.view(BITS[dtype]).fill_(PATTERN[dtype])
        self.view = self.buf[self.g:self.g + n].view(*shape)
        self.dtype, self.n = dtype, n
        if init is not None:
            self.view.copy_(init.reshape(shape).to(dtype))

    def read(self, name, all_written=True):
        """the owned elements as float64 on the CPU, after checking the guards (and that no owned element still holds the pattern)"""
        bits = self.buf.view(BITS[self.dtype])
        lo, own, hi = bits[:self.g], bits[self.g:self.g + self.n], bits[self.g + self.n:]
        p = PATTERN[self.dtype]
        assert bool((lo == p).all()) and bool((hi == p).all()), f"{name}: written outside the output ({int((lo != p).sum())} elements " \
                                                                 f"before, {int((hi != p).sum())} after)"
        if all_written:
            left = own == p
            assert not bool(left.any()), f"{name}: {int(left.sum())} owned elements never written, first at flat index {int(left.nonzero()[0])}"
        return c64(self.view)


def dev16(t):
    return t.to(torch.bfloat16).cuda().contiguous()


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ the kernels behind the runner interface
class Kernels:
    """gemm / wgrad as test_gemm_ref_cpu.Emulator has them: a spec of float64 tensors in, float64 results out"""

    def __init__(self, hip):
        self.hip = hip

    # -- rt_conv_gemm
    def launch(self, spec, group=None):
        hip, e = self.hip, spec["epi"]
        B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = spec["geom"]
        M = B * DH * DW
        opt16 = lambda k: dev16(e[k]) if e.get(k) is not None else None      # noqa: E731
        o32 = Guarded((M, N), torch.float32, init=e["res_f32"] if spec["alias"] else None) if "out_f32" in spec["stores"] else None
        o16 = Guarded((M, N), torch.bfloat16) if "out_bf16" in spec["stores"] else None
        op = Guarded((M, N), torch.bfloat16) if spec["out_preact"] else None
        acc2 = Guarded((M, N), torch.float32, init=e["acc2"]) if e.get("acc2") is not None else None
        res32 = o32.view if spec["alias"] else (dev32(e["res_f32"]) if e.get("res_f32") is not None else None)
        seed_dev = torch.tensor([e["seed_dev"]], dtype=torch.int64).to(torch.int32).cuda() if e.get("seed_dev") is not None else None
        hip.set_seed_dev(seed_dev)
        try:
            hip.conv_gemm(dev16(spec["src"]), dev16(spec["wgt"]), geom=spec["geom"], bias=dev32(e["bias"]) if e.get("bias") is not None else None,
                          res_f32=res32, res_bf16=opt16("res_bf16"), gate=opt16("gate"), gate_scale=e["gate_scale"], preact=opt16("preact"),
                          dtanh=opt16("dtanh"), res_first=e["res_first"], act=e["act"], drop_p=e.get("drop_p", 0.0), drop_seed=e.get("drop_seed", 0),
                          drop_shift=e.get("drop_shift", 0), transposed=spec["transposed"], out_bf16=o16.view if o16 is not None else False,
                          out_f32=o32.view if o32 is not None else False,
                          out_preact=op.view if op is not None else False, tile_hint=spec["hint"], group=group,
                          acc2_f32=acc2.view if acc2 is not None else None, dil=spec["dil"])
        finally:
            hip.set_seed_dev(None)
        return dict(out_f32=o32, out_bf16=o16, out_preact=op, acc2=acc2, keep=(seed_dev, res32))

    @staticmethod
    def collect(pending):
        torch.cuda.synchronize()
        return {k: v.read(k) for k, v in pending.items() if isinstance(v, Guarded)}

    def gemm(self, spec):
        return self.collect(self.launch(spec))

    # -- rt_conv_wgrad
    def launch_wgrad(self, spec, batch=None):
        hip = self.hip
        B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = spec["geom"]
        nk = N * KH * KW * SC
        dw = Guarded((nk,), torch.float32, init=None if spec["overwrite"] else spec["dw_before"])      # overwrite: dw holds the poison
        twin = Guarded((nk,), torch.bfloat16) if spec["g16"] else None
        db = Guarded((N,), torch.float32, init=spec["dbias_before"]) if spec["dbias_before"] is not None else None
        slots = torch.zeros(hip.SQ_SLOTS * hip.SQ_STRIDE, device="cuda") if spec["sq"] else None
        key = dw.view.data_ptr()
        if slots is not None:
            hip._SQACC_MAP[key] = (weakref.ref(self), slots)
        if twin is not None:
            hip._G16_MAP[key] = (weakref.ref(self), twin.view.data_ptr())
        dy, x = dev16(spec["dy"]).view(-1, N), dev16(spec["x"])
        scale = dev32(spec["scale"]) if spec["scale"] is not None else None
        try:
            if batch is None:
                hip.conv_wgrad(dy, x, dw.view, geom=spec["geom"], scale=scale, msplit=spec["msplit"], dbias=db.view if db is not None else None,
                               variant=spec["variant"], workspace=spec["workspace"], overwrite=spec["overwrite"], dil=spec["dil"])
            else:
                assert spec["msplit"] == 0 and spec["variant"] == 0
                batch.add_conv(dy, x, dw.view, spec["geom"], scale=scale, overwrite=spec["overwrite"], dil=spec["dil"],
                               dbias=db.view if db is not None else None)
        finally:
            hip._SQACC_MAP.pop(key, None); hip._G16_MAP.pop(key, None)
        return dict(dw=dw, g16=twin, dbias=db, slots=slots, keep=(dy, x, scale))

    def collect_wgrad(self, pending):
        torch.cuda.synchronize()
        out = {k: v.read(k) for k, v in pending.items() if isinstance(v, Guarded)}
        if pending["slots"] is not None:
            s = c64(pending["slots"]).view(self.hip.SQ_SLOTS, self.hip.SQ_STRIDE)
            assert float(s[:, 1:].abs().sum()) == 0.0, "sqacc: a word between the slots was written"
            out["sq"] = float(s[:, 0].sum())
        return out

    def wgrad(self, spec):
        return self.collect_wgrad(self.launch_wgrad(spec))


class Replay:
    """results already read back (a grouped launch's), handed to the check functions"""

    def __init__(self, got):
        self.got = got

    def gemm(self, spec):
        return self.got

    wgrad = gemm


def run_specs(hip, specs, check):
    w, n = Worst(), 0
    run = Kernels(hip)
    for tag, spec, exact in specs:
        check(w, run, spec, exact, tag)
        n += 1
    return w, n


# ------------------------------------------------------------------------------------------------ 1. tile forms
@pytest.mark.parametrize("hint", sorted(G.TILES))
def test_tile_forms(hip, hint):
    """M one short of a tile and two tiles + 5, N four and eight past a tile, K of one tile / as many as stages / one more / 2304,
    bias, both stores: tier 1 bit-exact, tier 2 inside the bounds"""
    assert hint in hip.PRODUCT_TILE_HINTS
    w, n = run_specs(hip, tile_specs(hint, KINDS), check_gemm)
    print(w.line(f"tile forms, hint {hint}, {n} products"))


# ------------------------------------------------------------------------------------------------ 2. the other routes
def test_skinny_route_and_first_tile_route(hip):
    """hint 0 at M = 16 (skinny_gemm_kernel) and at M = 17 with the same weights (the first tile route): row 16 is new, rows 0 .. 15
    the same exact values"""
    w = Worst()
    run = Kernels(hip)
    for kind in KINDS:
        for K, N in ((64, 68), (256, 72), (2304, 264)):
            g = torch.Generator().manual_seed(K + N)
            s17 = gemm_spec(kind, linear_geom(17, K, N), g, combo="bottleneck tail: bias + res_bf16 first + relu")
            s16 = dict(s17, src=s17["src"][:16], geom=linear_geom(16, K, N),
                       epi={k: (v[:16] if torch.is_tensor(v) and v.dim() == 2 else v) for k, v in s17["epi"].items()})
            a, _ = check_gemm(w, run, s16, kind == "ints", f"skinny 16x{K}x{N} {kind}")
            b, _ = check_gemm(w, run, s17, kind == "ints", f"tile 17x{K}x{N} {kind}")
            if kind == "ints":
                assert torch.equal(a["out_f32"], b["out_f32"][:16]) and torch.equal(a["out_bf16"], b["out_bf16"][:16])
    print(w.line("skinny and first tile route"))


GROUP_JOBS = [        # (M, K, N, combination): different row counts, widths and epilogues; the second is the aliased in-place form
    (333, 256, 264, "bottleneck tail: bias + res_bf16 first + relu"),
    (70, 128, 68, "in-place accumulation: gate, out_f32 is res_f32"),
    (129, 512, 72, "ffn hidden: bias + relu + dropout shift 2, seed_dev"),
]


@pytest.mark.parametrize("kind", EPI_KINDS)
def test_gemm_group_equals_single_launches_bit_for_bit(hip, kind):
    """three products of different M, N and epilogue in one rt_conv_gemm_grouped launch (dense, K < 1024, more than 16 rows, hint 0):
    each held like a single launch, and the same bits as the single launch"""
    w = Worst()
    run = Kernels(hip)
    specs = [gemm_spec(kind, linear_geom(M, K, N), torch.Generator().manual_seed(M + N), combo=c) for M, K, N, c in GROUP_JOBS]
    group = hip.GemmGroup()
    pend = [run.launch(s, group=group) for s in specs]
    group.run()
    grouped = [run.collect(p) for p in pend]
    for s, got, (M, K, N, c) in zip(specs, grouped, GROUP_JOBS):
        check_gemm(w, Replay(got), s, kind == "ints", f"grouped {M}x{K}x{N} {kind} [{c}]")
        single = run.gemm(s)
        for k in got:
            assert torch.equal(got[k], single[k]), (k, M, K, N)
    print(w.line(f"GemmGroup of three, {kind}"))


# ------------------------------------------------------------------------------------------------ 3. gathers
@pytest.mark.parametrize("hint", G.GATHER_HINTS)
def test_gathers_forward_and_transposed(hip, hint):
    w, n = run_specs(hip, gather_specs(hint, KINDS), check_gemm)
    print(w.line(f"gathers, hint {hint}, {n} products"))


PROBE_PIXELS = ((0, 0), (0, -1), (-1, 0), (-1, -1), (0, 0.5), (0.5, 0), (-1, 0.5), (0.5, -1), (0.5, 0.5), (0.34, 0.67))


@pytest.mark.parametrize("hint", G.GATHER_HINTS)
def test_one_hot_source_pixels(hip, hint):
    """One nonzero source pixel per image (value 1 in one channel), ten images: the four corners, the four edges, two interior
    pixels, the channel walking over the 64-wide K tiles.  Every output pixel is then one weight or zero: a wrong tap, pad, stride,
    dilation, divisibility test or tile offset is a whole wrong element.  Forward and transposed, every gather, bit-exact."""
    run = Kernels(hip)
    n = 0
    for i, name in enumerate(G.GATHERS):
        Ci, Co = (128, 64) if i % 2 == 0 else (64, 128)
        fwd, dil = G.conv_geom(name, Ci, Co)
        for tr in (False, True):
            geom = G.transposed_geom(fwd) if tr else fwd
            geom = (len(PROBE_PIXELS),) + geom[1:]
            spec = gemm_spec("ints", geom, torch.Generator().manual_seed(i), hint=hint, transposed=tr, dil=dil, combo={})
            SH, SW, SC = geom[1:4]
            src = torch.zeros_like(spec["src"])
            for b, (fy, fx) in enumerate(PROBE_PIXELS):
                y = int(fy * (SH - 1)) if fy >= 0 else SH - 1
                x = int(fx * (SW - 1)) if fx >= 0 else SW - 1
                src[b, y, x, (b * 37 + 63 * (b % 2)) % SC] = 1.0
            spec["src"] = src
            got, ref = check_gemm(Worst(), run, spec, True, f"one-hot hint {hint} {name} {'transposed' if tr else 'forward'}")
            assert int((ref.out != 0).sum()) > 0
            n += 1
    print(f"\n[one-hot source pixels, hint {hint}] {n} launches bit-exact")


# ------------------------------------------------------------------------------------------------ 4. epilogue combinations
@pytest.mark.parametrize("hint", [0] + sorted(G.TILES))
def test_epilogue_combinations(hip, hint):
    """every combination of gemm_ref.EPI_COMBOS (the model's call sites) with both stores on, at N % 8 = 4 (4-wide epilogue) and
    N % 8 = 0 (8-wide, LDS-staged, prefetched bf16 residual and gate): tier 1 where the combination is exact (there also with the
    bf16 and the fp32 store alone, as the call sites run them), tier 2 on two sets.
    Hint 0: the skinny route (M = 16) and the first tile route (M = 17)."""
    if hint == 0:
        specs = [s for M in (16, 17) for s in epilogue_specs(0, M, 128, (68, 72), EPI_KINDS)]
    else:
        specs = epilogue_specs(hint, *epilogue_shape(hint), EPI_KINDS)
    w, n = run_specs(hip, specs, check_gemm)
    print(w.line(f"epilogue combinations, hint {hint}, {n} products"))


# ------------------------------------------------------------------------------------------------ 5. weight gradients
@pytest.mark.parametrize("N,SC", G.WGRAD_NC)
def test_wgrad_first_generation(hip, N, SC):
    """M in {77, 200, 1000}; msplit 0, 1, 3 and more than the chunk count; workspace and atomics; overwrite and accumulate over a
    preloaded dw; scale; dbias; a registered sqacc and bf16 twin; the DMA kernels (variant 1) and the register-staged one (9)"""
    w, n = run_specs(hip, (s for s in wgrad_first_gen_specs(KINDS) if f"x{SC}->{N} " in s[0]), check_wgrad)
    print(w.line(f"first-generation weight gradients {SC} -> {N}, {n} launches"))


def test_wgrad_first_generation_gathers(hip):
    w, n = run_specs(hip, wgrad_gather_specs(KINDS), check_wgrad)
    print(w.line(f"first-generation weight gradients, gathers, {n} launches"))


@pytest.mark.parametrize("kind", KINDS)
def test_wgrad_second_generation_alone_and_grouped(hip, kind):
    """rt_wgrad2.hip at the smallest geometries rt_w2_eligible accepts (one with C % 16 = 8), each alone through rt_conv_wgrad, then
    all of them in one rt_conv_wgrad_grouped call together with a descriptor the group must forward (N % 8 = 4: first generation):
    held like the single launches; in tier 1 the same bits"""
    w = Worst()
    run = Kernels(hip)
    exact = kind == "ints"
    specs = [(name, w2_spec(name, kind, i % 2 == 0)) for i, name in enumerate(G.W2_CASES)]
    specs.append(("forwarded 200 x 80 -> 68", wgrad_spec(kind, linear_geom(200, 80, 68), torch.Generator().manual_seed(5))))
    # ... and two the first generation's own grouped kernel takes (N, SC >= 128, under 256 rows); the first-generation part of a
    # group has one norm accumulator per call: the forwarded descriptor's
    specs.append(("grouped v1 200 x 128 -> 128", wgrad_spec(kind, linear_geom(200, 128, 128), torch.Generator().manual_seed(6), sq=False, scale=False)))
    specs.append(("grouped v1 77 x 144 -> 136", wgrad_spec(kind, linear_geom(77, 144, 136), torch.Generator().manual_seed(7), sq=False, scale=False,
                                                           overwrite=True)))
    alone = [check_wgrad(w, run, s, exact, f"w2 alone {name} {kind}")[0] for name, s in specs]
    batch = hip.WgradBatch(workspace_mb=64)
    pend = [run.launch_wgrad(s, batch=batch) for _, s in specs]
    for d, p in zip(batch.descs, pend):              # (the maps are keyed by address: the descriptors carry what was registered)
        assert (d.sqacc or 0) == (p["slots"].data_ptr() if p["slots"] is not None else 0) and (d.g16 or 0) == p["g16"].view.data_ptr()
    batch.run()
    for (name, s), p, a in zip(specs, pend, alone):
        got = run.collect_wgrad(p)
        check_wgrad(w, Replay(got), s, exact, f"w2 grouped {name} {kind}")
        if exact:
            assert all(torch.equal(got[k], a[k]) for k in ("dw", "dbias", "g16")), name
    print(w.line(f"second-generation weight gradients alone and grouped, {kind}"))


@pytest.mark.parametrize("route", ["first generation", "second generation"])
def test_one_hot_dy_rows(hip, route):
    """One nonzero dy row (a single output pixel, integer channels): dw is that row's outer product with the gathered x row, every
    other row contributes nothing.  Rows: the first, the last, the edges of the 32-row chunks, an image boundary."""
    run = Kernels(hip)
    n = 0
    for name in G.WGRAD_GATHERS:
        if route == "first generation":
            geom, dil = G.conv_geom(name, 64, 68)                       # N % 8 = 4: the register-staged kernel
        else:
            B, H, W, Ci, Co, k, s, p, dil = G.W2_CASES[{"3x3 s1 p1": "3x3 s1 p1 fused taps", "3x3 s2 p1 odd": "3x3 s2 p1", "3x3 dil2 p2": "3x3 dil2 p2"}[name]]
            geom = (B, H, W, Ci, (H + 2 * p - dil * (k - 1) - 1) // s + 1, (W + 2 * p - dil * (k - 1) - 1) // s + 1, Co, k, k, s, p)
        M = geom[0] * geom[4] * geom[5]
        for m in sorted({0, 31, 32, M // 2 - 1, M // 2, M - 1}):
            spec = wgrad_spec("ints", geom, torch.Generator().manual_seed(m), dil=dil, overwrite=m % 2 == 0)
            dy = torch.zeros(M, geom[6], dtype=torch.float64)
            dy[m] = spec["dy"].reshape(M, -1)[m]
            spec["dy"] = dy.reshape(spec["dy"].shape)
            check_wgrad(Worst(), run, spec, True, f"one-hot dy row {m} {route} {name}")
            n += 1
    print(f"\n[one-hot dy rows, {route}] {n} launches bit-exact")
