"""GPU: the optimizer step of csrc/rt_optim.hip -- rt_sqnorm, rt_sqnorm_bf16, rt_adamw_flat, rt_sgd_flat, rt_adamw_chunks, rt_adamw_mat
with the bf16 operands and the state bytes it writes -- element by element against float64 (oracle/optim_ref.py, pinned to
torch.optim and its bounds proven usable on an fp32 emulation by tests/test_optim_ref_cpu.py, whose cases, operand sets and check
functions this file runs on the kernels).  The product library only.

Every buffer a launch may write (p, m, v, W, WT, the state bytes, gnorm_out) is a view of a larger buffer pre-filled with PATTERN, a
finite number: after each call the guards hold the pattern bit for bit, and every element the call does not own -- outside the span,
between chunks, between matrices -- holds the value it had.  The squared norm is computed on the host in float64 and passed in as the
fp32 word, so the order of the norm's atomics stays out of the element bounds; the norm kernels are held on their own.

Bounds (u = 2^-24, one u per fp32 rounding of the widest form of adam_elem, against sums of absolute values; see optim_ref):
  m' 2u |b1 m| + (4u + d_gs) |(1 - b1) g gs|      v' 2u b2 v + (6u + 2 d_gs) (1 - b2) (g gs)^2
  p' the bounds of m' and of the denominator through the quotient, the bias corrections with their amplification
     b^step / (1 - b^step), + (2 + lr wd) u |p| + u |p'|
  W, WT  bit for bit the bf16 image of the p' the kernel wrote; against the float64 p' its bound + 2^-8 |ref|
  norms  ((1 + u)^chain - 1) sum g^2, chain = 2063 .. 2076 roundings at the two large sizes (2048 atomics in any order)
sqrtf, the division, rsqrtf and powf: the host's error (1.05, 1.00, 1.50, 1.00 u) doubled for the device's math library.

Worst error / bound per tensor and path, measured on the MI355X (every test prints its own).  The bounds count one u per rounding,
so m and v, which take two to four roundings, come close to them; the flat pass on the device gives the figures of the CPU
emulation of its written-out fmas to the digit:
  rt_sqnorm / rt_sqnorm_bf16                       sq 0.03 / 0.08
  rt_adamw_flat, 5 sets x 8 variants x 6 steps     m 0.96  v 0.98  p 0.48  gnorm_out 0.28
      p at step 2 / step 7 alone                   0.47 / 0.48: the error of powf, amplified 499 and 142 times in 1 / sqrt(bc2), stays
                                                   inside the share one ulp of powf has in the bound -- no finding
  rt_adamw_flat, 4 Mi + 2052 elements              m 0.95  v 0.99  p 0.36  gnorm_out 0.17
  rt_sgd_flat, randn                               m 0.87  p 1.00 (its last fma rounds p' itself: half an ulp)  gnorm_out 0.16
  rt_sgd_flat, integers; the AdamW probes          bit-exact
  rt_adamw_chunks                                  m 0.49  v 0.50  p 0.48  gnorm_out 0.17
  rt_adamw_mat, vector path                        m 0.93  v 0.50  p 0.44  W 1.00  WT 1.00 (half a bf16 ulp); W, WT bits exact
  rt_adamw_mat, element-wise path                  m 0.53  v 0.62  p 0.27  W 0.89  WT 0.89; W, WT bits exact
  rt_adamw_chunks between the matrices             m 0.47  v 0.50  p 0.41
  rt_adamw_mat, sparse-state job, four steps       m 0.52  v 0.50  p 0.34  gnorm_out 0.29; state bytes equal after every step
Every guard intact, every unowned element unchanged, all refusals RT_ERR_BADARG with nothing written.  The whole file (62 tests, about
450 launches) takes 9 s on the MI355X; the slowest test is the 4 Mi case, 1.2 s.

Exact tiers, bit for bit on the device: three SGD steps on integers with power-of-two rates over eight ranges, a gap and a span;
AdamW with g = m = v = 0 and dyadic lr, wd (p' = p (1 - lr wd)) and with lr = 0 (p' keeps its bits), over all ranges at once, one
range at a time and inside the span.

Scratch mutations of csrc/rt_optim.hip (one line each, on a copy, not committed): the tests of this file that failed, and whether the
optimizer tests that existed before (test_ops_gpu.py, test_failsafe_gpu.py) did:
   1 eps added before the bias correction          flat 24 of 40 (all of eps, sharp, wide) + the 4 Mi case, chunks 6, matrix 4, sparse job;
                                                   before: test_sqnorm_adamw
   2 inv_sqrt_bc2 computed from beta1              flat 40 + 4 Mi, chunks 6, matrix 8, sparse job; before: test_sqnorm_adamw
   3 adam_range: e > range_begin[r]                flat 40 + 4 Mi, the exact probes, SGD 2, chunks 6, matrix 4, sparse job; before:
                                                   test_sqnorm_adamw, test_sgd_flat_matches_torch_sgd..., test_sparse_state_adamw_is_bit_exact...
   4 clip_scale: total without grad_scale          flat 5 (grad_scale 0.5), matrix 8; before: NOTHING
   5 adamw_kernel: stride gridDim.x * 255          the 4 Mi case; before: NOTHING
   6 sqnorm_kernel: no ragged-tail loop            both norm tests; before: NOTHING
   7 adam_coef: step_dev ignored                   flat 5 (step_dev) + 4 Mi, chunks 6, matrix 4 (bf16 gradients); before: NOTHING
   8 adamw_mat_kernel: G16 + o + 4                 matrix 4 (bf16 gradients); before: test_matrix_adamw_equals_flat_adamw_plus_weight_prep
   9 adam_elem: lr / bc1 made lr                   flat 40 + 4 Mi, chunks 6, matrix 8, sparse job; before: test_sqnorm_adamw
  10 state byte from m alone                       the sparse job (row 20: m = 0, v != 0); before: NOTHING
"""
import ctypes

import pytest
import torch

from oracle import optim_ref as R
from test_optim_ref_cpu import (N_FLAT, RANGES8, SPAN, VARIANTS, _adam_ref, adam_spec, check_adamw, check_sgd, dyadic_ranges, flat_specs,
                                hold_region, probe_spec, sgd_spec)
from test_region_fp64_gpu import Worst, c64, hold

pytestmark = pytest.mark.gpu

GUARD = 64                               # elements before and after every buffer a launch may write
PATTERN = {torch.bfloat16: 0x5A5B, torch.float32: 0x5A5B5A5B, torch.uint8: 0x5A}       # 1.5e16 in both float formats
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
BADARG = -1


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """`n` elements of `dtype` inside a larger buffer that holds PATTERN, then `init` if given.  shift: the view begins `shift`
    elements later (a view that is not 16-byte aligned); the elements in front of it count as guard."""

    def __init__(self, n, dtype, init=None, shift=0):
        self.g, self.n, self.dtype = GUARD + shift, n, dtype
        self.buf = torch.empty(n + 2 * GUARD + shift, dtype=dtype, device="cuda")
        self.buf.view(BITS[dtype]).fill_(PATTERN[dtype])
        self.view = self.buf[self.g:self.g + n]
        if init is not None:
            self.view.copy_(init.reshape(n).to(dtype))

    def read(self, name, all_written=False):
        """the owned elements as float64 on the CPU, after checking the guards"""
        bits = self.buf.view(BITS[self.dtype])
        lo, own, hi = bits[:self.g], bits[self.g:self.g + self.n], bits[self.g + self.n:]
        pat = PATTERN[self.dtype]
        assert bool((lo == pat).all()) and bool((hi == pat).all()), f"{name}: written outside the buffer ({int((lo != pat).sum())} elements " \
                                                                 f"before, {int((hi != pat).sum())} after)"
        if all_written:
            left = own == pat
            assert not bool(left.any()), f"{name}: {int(left.sum())} owned elements never written, first at {int(left.nonzero()[0])}"
        return c64(self.view)


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def dev16(t):
    return t.to(torch.bfloat16).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ the kernels behind the emulator's interface
class Kernels:
    """adamw / sgd as test_optim_ref_cpu.Emulator has them: a spec of float64 tensors in, the float64 buffers after the launch out"""

    def __init__(self, hip):
        self.hip = hip

    def launch(self, spec, *, sgd=False, steps=1, mat=None, chunks=None):
        hip, n = self.hip, spec["n"]
        P, M = Guarded(n, torch.float32, spec["p"]), Guarded(n, torch.float32, spec["m"])
        V = Guarded(4, torch.float32, torch.zeros(4)) if sgd else Guarded(n, torch.float32, spec["v"])
        gn = Guarded(1, torch.float32)
        g32 = None if spec["g16"] else dev32(spec["g"])                     # with a bf16 buffer the fp32 one is not there at all
        g16 = dev16(spec["g"]) if spec["g16"] else None
        sq = torch.tensor([spec["sq"]], dtype=torch.float64).float().cuda() if spec["sq"] is not None else None
        ranges, lr_dev, step_dev, step = spec["ranges"], None, None, spec["step"]
        if spec["lr_dev"]:                                                  # rates by value that the device words must override
            lr_dev = torch.tensor([r[2] for r in ranges] + [0.0] * (8 - len(ranges)), dtype=torch.float64).float().cuda()
            ranges = [(b, e, 7.0, w) for b, e, _, w in ranges]
        if spec["step_dev"]:                                                # a step by value that the device word must override
            step_dev, step = torch.tensor([spec["step"]], dtype=torch.int32).cuda(), spec["step"] + 5
        for _ in range(steps):
            hip.adamw_flat(P.view, g32, M.view, V.view, step=step, ranges=ranges, gnorm_sq=sq, gnorm_out=gn.view, grad_scale=spec["grad_scale"],
                           max_norm=spec["max_norm"], beta1=spec["beta1"], beta2=spec["beta2"], eps=spec["eps"], step_dev=step_dev, lr_dev=lr_dev,
                           span=spec["span"], g16=g16, sgd=sgd, mat=mat, chunks=chunks)
        torch.cuda.synchronize()
        out = dict(p=P.read("p"), m=M.read("m"), gnorm_out=float(gn.read("gnorm_out", all_written=True)))
        if sgd:
            assert float(V.read("v").abs().max()) == 0.0, "rt_sgd_flat wrote v"
        else:
            out["v"] = V.read("v")
        return out

    def adamw(self, spec, **kw):
        return self.launch(spec, **kw)

    def sgd(self, spec, steps=1):
        return self.launch(spec, sgd=True, steps=steps)


@pytest.fixture(scope="module")
def K(hip):
    return Kernels(hip)


# ------------------------------------------------------------------------------------------------ the norms
NORM_SIZES = {torch.float32: (1, 3, 7, 8, 9, 1027, 3 * 2 ** 20 + 5), torch.bfloat16: (1, 3, 7, 8, 9, 1027, 5 * 2 ** 20 + 11)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["rt_sqnorm", "rt_sqnorm_bf16"])
def test_squared_norm_at_ragged_sizes_and_past_the_workgroup_cap(hip, dtype):
    """n below one vector, n % 4 and n % 8 != 0, and a size past the 2048-workgroup cap with a ragged tail (two grid-stride
    iterations), on positive-biased values and on magnitudes spread over 2^-20 .. 2^8, at the chain bound of optim_ref.sqnorm_chain"""
    w = Worst()
    gen = torch.Generator().manual_seed(21)
    for n in NORM_SIZES[dtype]:
        for kind in ("biased", "wide"):
            x = torch.randn(n, generator=gen, dtype=torch.float64) + 3.0 if kind == "biased" else R.operands("wide", n, gen)[1]
            xd = x.to(dtype).cuda()
            out = Guarded(1, torch.float32)
            hip.sqnorm(xd, out.view)
            torch.cuda.synchronize()
            ref = c64(xd)
            want = torch.tensor([R.sqnorm_ref(ref)], dtype=torch.float64)
            hold(w, "sq", out.read("sq", all_written=True), want, R.sqnorm_bound(ref, dtype == torch.bfloat16))
    print(w.line("rt_sqnorm" if dtype == torch.float32 else "rt_sqnorm_bf16"))


# ------------------------------------------------------------------------------------------------ the flat pass
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", R.OPERAND_SETS)
def test_flat_adamw_per_element(K, kind, variant):
    """rt_adamw_flat over eight ranges and a gap at steps 1, 2, 7, 1000, 30000 and 120000 (powf(beta2, step) underflows)"""
    w = Worst()
    for spec in flat_specs(kind, variant):
        ws = Worst()
        check_adamw(ws, "flat ", spec, K.adamw(spec))
        for k, v in ws.items():
            w.note(k, v)
        if spec["step"] in (2, 7):
            w.note(f"flat p at step {spec['step']}", ws["flat p"])
    print(w.line(f"rt_adamw_flat {kind}, {variant}"))


N_BIG = 4 * 2 ** 20 + 2052
_BIG = {}


def big_case():
    """4 Mi + 2052 elements of the sharp set, two ranges: 4097 workgroups' worth, so the 4096 launched run the grid-stride loop twice.
    The spec and its float64 reference are computed once per module."""
    if not _BIG:
        spec = adam_spec("sharp", N_BIG, 9, 7, [(0, 2 * 2 ** 20 + 1028, 1e-4, 1e-4), (2 * 2 ** 20 + 1028, N_BIG, 3e-5, 0.0)], step_dev=True)
        _BIG.update(spec=spec, ref=_adam_ref(spec))
    return _BIG["spec"], _BIG["ref"]


def test_flat_adamw_past_the_workgroup_cap(K):
    spec, ref = big_case()
    w = Worst()
    check_adamw(w, "flat, grid-stride ", spec, K.adamw(spec), ref)
    print(w.line("rt_adamw_flat, 4 Mi + 2052 elements"))


def _edges(spec):
    """the first and last four elements of each range and of the span"""
    idx = []
    for b, e in [(r[0], r[1]) for r in spec["ranges"]] + [spec["span"] or (0, spec["n"])]:
        idx += list(range(b, b + 4)) + list(range(e - 4, e))
    return torch.tensor(sorted(set(idx)))


def test_flat_adamw_exact_probes(K):
    """g = m = v = 0: p' = p (1 - lr wd) with dyadic lr, wd, and p' = p bit for bit with lr = 0, have one legal value.  All ranges at
    once, inside the span, and one range at a time (the others then have lr = wd = 0 and keep their bits)."""
    w = Worst()
    specs = [(f"{'lr 0' if z else 'decay'}{', span' if sp else ''} ", probe_spec(N_FLAT, dyadic_ranges(RANGES8), lr_zero=z, span=sp))
             for z in (False, True) for sp in (None, SPAN)]
    specs += [(f"range {r} alone ", probe_spec(N_FLAT, dyadic_ranges(RANGES8, only=r))) for r in range(len(RANGES8))]
    for tag, spec in specs:
        got = K.adamw(spec)
        ref = check_adamw(w, tag, spec, got)
        e = _edges(spec)
        want = torch.where(spec["own"], ref.p, spec["p"])
        assert torch.equal(got["p"][e], want[e]), f"{tag}: the first or last four elements of a range or of the span"
    assert all(v == 0.0 for v in w.values()), w


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("kind", ["randn", "ints"])
def test_flat_sgd_exact_tier_and_per_element(K, kind):
    """rt_sgd_flat: three steps on integers with power-of-two rates and momentum 0.5 bit for bit; the randn set at the bound of
    sgd_ref.  Eight ranges and the gap; the whole buffer, the span, bf16 gradients."""
    w = Worst()
    for variant in ("plain", "span (4100, 8200)", "bf16 gradients"):
        kw = {k: v for k, v in VARIANTS[variant].items() if k in ("span", "g16")}
        spec = sgd_spec(kind, N_FLAT, 31, RANGES8, clip="off" if kind == "ints" else "engaged", **kw)
        steps = 3 if kind == "ints" else 1
        got = K.sgd(spec, steps)
        check_sgd(w, "sgd ", spec, got, steps)
        c = spec["clip"]
        hold(w, "sgd gnorm_out", torch.tensor([got["gnorm_out"]], dtype=torch.float64), torch.tensor([c.total], dtype=torch.float64), c.bound_total)
    print(w.line(f"rt_sgd_flat {kind}"))
    if kind == "ints":
        assert w["sgd m"] == 0.0 and w["sgd p"] == 0.0


# ------------------------------------------------------------------------------------------------ chunks
CHUNKS = [(0, 4), (8, 16384), (16400, 1020), (17424, 16384)]
N_CHUNKS = 33812


def _mask(n, pieces):
    own = torch.zeros(n, dtype=torch.bool)
    for off, cnt in pieces:
        own[off:off + cnt] = True
    return own


@pytest.mark.parametrize("g16", [False, True], ids=["fp32 gradients", "bf16 gradients"])
@pytest.mark.parametrize("kind", ["randn", "sharp", "eps"])
def test_chunk_adamw_per_element(K, kind, g16):
    """rt_adamw_chunks over a table with a four-element chunk, two full ones and a short one; elements 4 .. 7, 16392 .. 16399 and
    17420 .. 17423 lie outside every chunk.  The step comes from step_dev."""
    own = _mask(N_CHUNKS, CHUNKS)
    assert not own[4:8].any() and not own[16392:16400].any() and not own[17420:17424].any() and int((~own).sum()) == 4 + 8 + 4 + 4
    ranges = [(0, 8200, 1e-4, 1e-4), (8200, 17428, 3e-5, 0.0), (17428, N_CHUNKS, 2e-4, 1e-2)]
    tab = torch.tensor([x for c in CHUNKS for x in c], dtype=torch.int64).cuda()
    w = Worst()
    for i, step in enumerate((1, 7, 1000)):
        spec = adam_spec(kind, N_CHUNKS, 300 + i, step, ranges, own=own, g16=g16, step_dev=True)
        check_adamw(w, "chunks ", spec, K.adamw(spec, chunks=(tab, len(CHUNKS))))
    print(w.line(f"rt_adamw_chunks {kind}"))


# ------------------------------------------------------------------------------------------------ matrix tiles
# N, T, C, FrozenBN scale, dst, dst_t, elements dst_t is shifted off its alignment
MATS = [(192, 1, 128, False, True, True, 1),       # vector path; the transposed copy lands on a view that is not 16-byte aligned
        (72, 9, 64, True, True, True, 0),          # a 3x3 convolution with a FrozenBN scale; N % 8 == 0: 16-byte transposed stores
        (10, 1, 12, False, False, True, 0),        # K no multiple of 256; dst_t alone
        (20, 1, 260, False, True, True, 0),        # K % 4 == 0 with a partial column tile, N % 8 != 0: the transposed copy element-wise
        (33, 1, 256, False, True, False, 0),       # a second row tile that holds one row; dst alone
        (7, 1, 10, False, True, True, 0)]          # K % 4 != 0: the element-wise path
GAPS = (256, 40, 8, 12, 36, 4096 + 36)             # loose vectors in front of each matrix


def _mat_layout():
    """offsets of MATS in one buffer.  cover_span asks N T C % 4 == 0 of a matrix, which 7 x 1 x 10 is not: it lies behind the span
    that cover_span tiles, as a job of its own, followed by 2 + 8 elements that nothing owns."""
    offs, pos = [], 0
    for gap, (N, T, C, *_) in zip(GAPS, MATS):
        pos += gap
        offs.append(pos)
        pos += N * T * C
    return offs, offs[-1], pos + 2 + 8


@pytest.mark.parametrize("with_chunks", [False, True], ids=["matrices alone", "matrices and chunks"])
@pytest.mark.parametrize("g16", [False, True], ids=["fp32 gradients", "bf16 gradients"])
@pytest.mark.parametrize("kind", ["randn", "sharp"])
def test_matrix_adamw_per_element_and_its_operands(hip, K, kind, g16, with_chunks):
    """rt_adamw_mat over six matrices with loose vectors between them (reftr_amd.optim.cover_span), alone -- the loose vectors must
    keep their bits -- and with rt_adamw_chunks over the complement.  m', v', p' at the bounds; W and WT bit for bit the bf16 image
    of the p' the kernel wrote, and within the bound of p' + 2^-8 |ref| of the float64 p'."""
    from reftr_amd.optim import cover_span
    offs, e, n = _mat_layout()
    gen = torch.Generator().manual_seed(41)
    scale = R.r32(torch.rand(72, generator=gen, dtype=torch.float64) + 0.5)
    scale_d = dev32(scale)
    jobs, tiles, chunks = cover_span([(o, N, T, C) for o, (N, T, C, *_) in zip(offs[:-1], MATS[:-1])], 0, e)
    N, T, C = MATS[-1][:3]
    jobs.append((offs[-1], N, T, C, tiles))
    tiles += ((N + 31) // 32) * ((T * C + 255) // 256)
    ops, rows = [], []
    for (off, N, T, C, first), (_, _, _, sc, dst, dst_t, shift) in zip(jobs, MATS):
        W = Guarded(N * T * C, torch.bfloat16) if dst else None
        WT = Guarded(N * T * C, torch.bfloat16, shift=shift) if dst_t else None
        assert WT is None or (WT.view.data_ptr() % 16 != 0) == (shift != 0)
        rows.append([off, scale_d.data_ptr() if sc else 0, W.view.data_ptr() if W else 0, WT.view.data_ptr() if WT else 0, N, T, C, first])
        ops.append((W, WT))
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    ctab = torch.tensor(chunks, dtype=torch.int64).cuda()
    regions = [(o, N * T * C) for o, (N, T, C, *_) in zip(offs, MATS)]
    own = _mask(n, regions)
    if with_chunks:
        own[:e] = True
    ranges = [(0, offs[1] - 20, 1e-3, 1e-4), (offs[1] - 20, n, 1e-4, 0.0)]          # the boundary lies in the loose vector between two matrices
    spec = adam_spec(kind, n, 400, 3, ranges, own=own, g16=g16, step_dev=g16, grad_scale=0.5)
    got = K.adamw(spec, mat=(tab, len(rows), tiles), chunks=(ctab, len(chunks) // 2) if with_chunks else None)
    w = Worst()
    ref = check_adamw(Worst(), "", spec, got)
    for (off, cnt), (N, T, C, sc, *_), (W, WT) in zip(regions, MATS, ops):
        path = "vector" if (T * C) % 4 == 0 else "element-wise"
        region = _mask(n, [(off, cnt)])
        hold_region(w, f"{path} ", spec, got, ref, region)
        image = R.operands_ref(got["p"][off:off + cnt], N, T, C, scale if sc else None)
        exact = R.operands_exact(ref.p[off:off + cnt], ref.bound_p[off:off + cnt], N, T, C, scale if sc else None)
        for name, buf, img, ex, bound in (("W", W, image[0], exact[0], exact[2]), ("WT", WT, image[1], exact[1], exact[3])):
            if buf is None:
                continue
            o = buf.read(f"{name} of {N}x{T}x{C}", all_written=True)
            hold(w, f"{path} {name} bits", o, img.reshape(-1), 0.0)
            hold(w, f"{path} {name}", o, ex.reshape(-1), bound.reshape(-1))
    if with_chunks:
        hold_region(w, "chunks between ", spec, got, ref, own & ~_mask(n, regions))
    print(w.line(f"rt_adamw_mat {kind}"))


def test_sparse_state_job_per_element_and_its_state_bytes(hip, K):
    """A 100 x 1 x 768 job with state bytes (one per KB row piece, 0 = `m and v of this piece are all zero`), four steps with rows
    entering late and one step without any gradient.  Each step is held against float64 from the state the kernel left, and the
    bytes after it equal `m' != 0 | v' != 0` of the float64 reference, piece by piece.  Row 20 has m = 0, v != 0 and never a gradient:
    its bytes must stay 1, since v alone is state.

    Not run: a row with m, v != 0 whose byte is 0.  A byte of 0 is the kernel's own statement that it left m = v = 0 there; the host
    resets the bytes to 1 (unknown) whenever m or v are written from outside (FusedAdamW's version check,
    test_sparse_state_bytes_follow_moments_written_from_outside).  A cleared byte beside live moments is therefore no legal input:
    the kernel would skip the piece, by design."""
    N, Kc = 100, 768
    n, kt = N * Kc, 3
    tiles = ((N + 31) // 32) * kt
    gen = torch.Generator().manual_seed(43)
    p = R.r32(torch.randn(n, generator=gen, dtype=torch.float64))
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    v.view(N, Kc)[20] = R.r32(torch.rand(Kc, generator=gen, dtype=torch.float64) * 1e-3 + 1e-6)
    flags = Guarded(N * kt, torch.uint8, torch.ones(N * kt))
    P, M, V = (Guarded(n, torch.float32, t) for t in (p, m, v))
    gn = Guarded(1, torch.float32)
    tab = torch.tensor([[0, flags.view.data_ptr(), 0, 0, N, 1, Kc, 0]], dtype=torch.int64).cuda()
    ranges = [(0, n, 1e-5, 1e-4)]                     # 1 - lr wd rounds to 1: the skip is taken
    w = Worst()
    for step, rows in enumerate(([3, 50], [3], [], [77, 50]), start=1):
        gr = torch.zeros(N, Kc, dtype=torch.float64)
        for r in rows:
            gr[r] = torch.randn(Kc, generator=gen, dtype=torch.float64) * 0.1
        if step == 4:
            gr[12, 300:310] = 0.5                     # a single piece of a row
        gr = R.r32(gr.reshape(-1))
        spec = adam_spec("randn", n, 0, step, ranges)
        sq = R.f32(R.sqnorm_ref(gr))
        spec.update(p=P.read("p"), g=gr, m=M.read("m"), v=V.read("v"), sq=sq, max_norm=R.f32(0.1), clip=R.clip_ref(sq, 1.0, 0.1))
        hip.adamw_flat(P.view, dev32(gr), M.view, V.view, step=step, ranges=ranges, gnorm_sq=torch.tensor([sq], dtype=torch.float64).float().cuda(),
                       gnorm_out=gn.view, max_norm=0.1, mat=(tab, 1, tiles))
        torch.cuda.synchronize()
        got = dict(p=P.read("p"), m=M.read("m"), v=V.read("v"), gnorm_out=float(gn.read("gnorm_out")))
        ref = check_adamw(w, "sparse ", spec, got)
        live = ((ref.m != 0) | (ref.v != 0)).view(N, kt, 256).any(dim=2)
        assert torch.equal(flags.read("state bytes").view(N, kt) != 0, live), f"state bytes after step {step}"
        assert bool(live[20].all())
    assert int(live.sum()) == 3 * 4 + 1                # rows 3, 50, 77 and 20 whole, one piece of row 12
    assert torch.equal(got["p"].view(N, Kc)[0], p.view(N, Kc)[0])         # an untouched row never moved
    print(w.line("rt_adamw_mat, sparse-state job"))


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_descriptors_are_refused_before_any_launch(hip):
    """Each descriptor below is answered with RT_ERR_BADARG by the argument check, before any launch, and every buffer keeps its
    bits.  (No test that existed before asserts any refusal of the four update entries.)"""
    n = 4096
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(n, generator=gen) for _ in range(3)]
    P, M, V = (Guarded(n, torch.float32, t) for t in init)
    gn = Guarded(1, torch.float32)
    g = torch.randn(n, generator=gen).cuda()
    tab = torch.tensor([0, 1024], dtype=torch.int64).cuda()
    mtab = torch.tensor([[0, 0, 0, 0, 32, 1, 128, 0]], dtype=torch.int64).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(p=P.view, g=g, m=M.view, v=V.view, n=n, gnorm_out=gn.view, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, step=1, n_ranges=1,
                range_begin=(0,), range_end=(n,), range_lr=(1e-3,), range_wd=(1e-2,))
    bad = {"n % 4 != 0": dict(n=n - 2, range_end=(n - 4,)),
           "a range begin that is no multiple of 4": dict(range_begin=(2,)),
           "a range end that is no multiple of 4": dict(range_end=(n - 2,)),
           "no range": dict(n_ranges=0),
           "nine ranges": dict(n_ranges=9),
           "step 0 without step_dev": dict(step=0),
           "a span begin that is no multiple of 4": dict(span_begin=2, span_end=n),
           "a span end that is no multiple of 4": dict(span_begin=4, span_end=n - 2),
           "a span past n": dict(span_begin=4, span_end=n + 4),
           "begin == end": dict(span_begin=64, span_end=64),
           "begin > end": dict(span_begin=128, span_end=64)}
    lib = hip.lib()
    calls = {"rt_adamw_flat": lambda d: lib.rt_adamw_flat(ctypes.byref(d), stream),
             "rt_sgd_flat": lambda d: lib.rt_sgd_flat(ctypes.byref(d), stream),
             "rt_adamw_chunks": lambda d: lib.rt_adamw_chunks(ctypes.byref(d), tab.data_ptr(), 1, stream),
             "rt_adamw_mat": lambda d: lib.rt_adamw_mat(ctypes.byref(d), mtab.data_ptr(), 1, 1, stream)}
    for name, call in calls.items():
        for what, fields in bad.items():
            if fields.keys() & {"span_begin", "span_end"} and name in ("rt_adamw_chunks", "rt_adamw_mat"):
                continue                                  # the tables say what is updated: these two entries do not read the span
            if "step" in fields and name == "rt_sgd_flat":
                continue                                  # SGD has no step
            rc = call(hip._desc(hip.AdamWDesc, **{**good, **fields}))
            assert rc == BADARG, f"{name}: {what}: returned {rc}"
    torch.cuda.synchronize()
    for buf, t, name in ((P, init[0], "p"), (M, init[1], "m"), (V, init[2], "v")):
        assert torch.equal(buf.read(name), t.double()), name
    assert int(gn.buf.view(torch.int32)[GUARD]) == PATTERN[torch.float32], "gnorm_out was written"
    # the descriptor itself is sound: the same fields are accepted
    assert calls["rt_adamw_flat"](hip._desc(hip.AdamWDesc, **good)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(P.read("p"), init[0].double())
