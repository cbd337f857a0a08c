"""CPU: oracle/gemm_ref.py, the float64 reference and the element-wise bounds tests/test_gemm_fp64_gpu.py holds rt_conv_gemm /
rt_conv_wgrad to.

  1. the reference against float64 autograd through F.conv2d (forward, backward-data, weight gradient; no conv_transpose) at every
     geometry of gemm_ref.GATHERS -- stride 2 on odd sizes, dil 2 and 3, pad 0 / 1 / dil -- to 1e-12 relative
  2. the dropout decisions against the numpy hash_keep of tests/test_gemm_gpu.py, with drop_shift, and the seed_dev form against
     rt_site_seed's definition
  3. the activation constants of gemm_ref.ACT_MEASURED re-measured
  4. the bounds hold for a CPU emulation that accumulates in fp32 in adversarial orders (forward, reversed, per 32-wide step, K split
     four ways; weight gradients: split-M partials summed last) and rounds to bf16 where the kernels round: every error / bound
     <= 1, no element left out, through the check functions the GPU file runs on the kernels (cases, inputs and checks below are
     the GPU file's too); tier 1 (integer operands) is bit-exact in every order

Worst error / bound of the emulator over all cases, operand sets and orders (each test prints its own):
  tile forms   out_f32 0.02, out_bf16 0.99
  gathers      out_f32 0.01, out_bf16 0.98
  epilogues    out_f32 0.09, out_bf16 0.99, out_preact 0.98, acc2 0.01
  wgrad        dw 0.01, dbias 0.00, g16 0.99, sq 0.00
(bf16 stores come close to 1: half an ulp of a value just above a power of two is 2^-8 of it.  The fp32 bounds are worst-case over
every order and sign pattern; random operands use a few per cent of them -- tier 1 is the sharp check of fp32 values.)
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gemm_ref as G
from test_gemm_gpu import hash_keep
from test_region_fp64_gpu import Worst, hold, pbound

ORDERS = ("forward", "reversed", "step32", "ksplit4")


# ------------------------------------------------------------------------------------------------ specs (shared with the GPU file)
def gemm_spec(kind, geom, g, *, hint=0, transposed=False, dil=1, combo=None, exact=None):
    """One rt_conv_gemm problem: operands of set `kind` (gemm_ref.operand_pair), the epilogue of `combo` (bias alone when None)"""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    exact = (kind == "ints") if exact is None else exact
    src, wgt = G.operand_pair(kind, (B, SH, SW, SC), (N, KH, KW, SC), 3, 3, KH * KW * SC, g)
    epi, out_preact, alias = G.epilogue_tensors(combo if combo is not None else dict(bias=1), B * DH * DW, N, g, exact)
    return dict(src=src, wgt=wgt, geom=geom, transposed=transposed, dil=dil, hint=hint, epi=epi, out_preact=out_preact, alias=alias,
                stores=("out_f32", "out_bf16"))


def single_store(spec):
    """the spec with one store only, as most call sites run it (the epilogue branches on each destination): bf16, and fp32 too"""
    return [dict(spec, stores=(k,)) for k in ("out_bf16", "out_f32") if not (spec["alias"] and k == "out_bf16")]


def linear_geom(M, K, N):
    return (M, 1, 1, K, 1, 1, N, 1, 1, 1, 0)


def wgrad_spec(kind, geom, g, *, dil=1, scale=True, overwrite=False, msplit=0, workspace=True, variant=0, dbias=True, sq=True, g16=True):
    """One rt_conv_wgrad problem; the contraction runs over the rows: `cancel` pairs the two halves of the batch axis"""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    exact = kind == "ints"
    x, dy = G.operand_pair(kind, (B, SH, SW, SC), (B, DH, DW, N), 0, 0, 1, g)       # (a gathered problem: the images meet tap by tap)
    M = B * DH * DW
    S = min(msplit, -(-M // 32)) if msplit > 0 else max(1, -(-M // 256))
    pw2 = 2.0 ** torch.randint(-2, 3, (N,), generator=g).double()
    return dict(dy=dy, x=x, geom=geom, dil=dil, overwrite=overwrite, msplit=msplit, workspace=workspace, variant=variant, sq=sq, g16=g16,
                scale=(pw2 if exact else (torch.rand(N, generator=g) + 0.5).float().double()) if scale else None,
                dw_before=G.ints((N, KH * KW * SC), g) if exact else torch.randn(N, KH * KW * SC, generator=g).float().double(),
                dbias_before=(G.ints((N,), g) if exact else torch.randn(N, generator=g).float().double()) if dbias else None,
                # S of the bound: the partial tiles the split reduction adds.  An explicit msplit gives at most min(msplit, chunks)
                # partials (wg_set_splits, chunks of >= 32 rows); left to the library, the first generation cuts splits of >= 256
                # rows (wg_dma_auto_split; the register-staged kernel >= 512) and so does the second (w2_plan: maxs = M / 256)
                splits=S)


# ------------------------------------------------------------------------------------------------ checks (shared with the GPU file)
def same(name, got, ref, dtype):
    """every element equal to the exact value rounded once to `dtype` (the operands are integers: nothing else is a legal result);
    compared as values, so -0 and +0 agree and the poison pattern, a finite number, never does"""
    ref = ref.to(torch.float32).to(dtype).double()
    got = got.reshape(ref.shape)
    bad = got != ref
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        idx = np.unravel_index(i, tuple(ref.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first {idx}: got {float(got.reshape(-1)[i])!r} "
                             f"exact {float(ref.reshape(-1)[i])!r}")


def check_gemm(w, run, spec, exact, tag=""):
    """out_f32 and out_bf16 (spec["stores"]: both unless single_store made it one), out_preact and acc2 of one product against
    gemm_ref.conv_gemm_ref"""
    ref = G.conv_gemm_ref(spec["src"], spec["wgt"], spec["geom"], transposed=spec["transposed"], dil=spec["dil"], **spec["epi"])
    got = run.gemm(spec)
    items = [("out_f32", ref.out, ref.bound, torch.float32), ("out_bf16", ref.out, ref.bound + G.U16 * ref.out.abs(), torch.bfloat16)]
    items = [it for it in items if it[0] in spec["stores"]]
    if spec["out_preact"]:
        items.append(("out_preact", ref.out_preact, ref.bound_preact + G.U16 * ref.out_preact.abs(), torch.bfloat16))
    if ref.acc2 is not None:
        items.append(("acc2", ref.acc2, ref.bound_acc2, torch.float32))
    for name, r, bound, dtype in items:
        if exact:
            same(f"{tag} {name}", got[name], r, dtype)
        else:
            try:
                hold(w, name, got[name], r, bound)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
    return got, ref


def check_wgrad(w, run, spec, exact, tag=""):
    """dw, dbias, the bf16 twin and the sqacc increment of one weight gradient against gemm_ref.conv_wgrad_ref"""
    ref = G.conv_wgrad_ref(spec["dy"], spec["x"], spec["geom"], dw_before=spec["dw_before"], scale=spec["scale"], overwrite=spec["overwrite"],
                           dil=spec["dil"], dbias_before=spec["dbias_before"], splits=spec["splits"])
    got = run.wgrad(spec)
    items = [("dw", ref.dw, ref.bound, torch.float32)]
    if spec["dbias_before"] is not None:
        items.append(("dbias", ref.dbias, ref.bound_dbias, torch.float32))
    if spec["g16"]:
        items.append(("g16", ref.dw, ref.bound + G.U16 * ref.dw.abs(), torch.bfloat16))
    for name, r, bound, dtype in items:
        if exact:
            same(f"{tag} {name}", got[name], r, dtype)
        else:
            try:
                hold(w, name, got[name], r, bound)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
    if spec["sq"]:
        # teacher-forced: the increment the kernel's OWN dw implies (its distance to the exact dw is held above)
        after = got["dw"].reshape(ref.dw.shape)
        sq = torch.tensor([float((after * after).sum() - (ref.before * ref.before).sum())], dtype=torch.float64)
        try:
            hold(w, "sq", torch.tensor([got["sq"]], dtype=torch.float64), sq, G.sq_bound(after, ref.before))
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
    return got, ref


# ------------------------------------------------------------------------------------------------ the emulator
def _accumulate(a, b, order):
    """sum_k a[:, k] b[:, k]^T -> [Ma, Mb] with every addition rounded to fp32 in the given order (products of bf16 values: exact)"""
    a32, b32 = a.float(), b.float()
    K = a.shape[1]
    if order in ("forward", "reversed"):
        acc = torch.zeros(a.shape[0], b.shape[0])
        for k in (range(K) if order == "forward" else range(K - 1, -1, -1)):
            acc += a32[:, k:k + 1] * b32[:, k][None, :]
        return acc
    if order == "step32":            # one MFMA step: 32 products added exactly, rounded once, then the running sum
        acc = torch.zeros(a.shape[0], b.shape[0])
        for k in range(0, K, 32):
            acc += (a[:, k:k + 32] @ b[:, k:k + 32].t()).float()
        return acc
    q = -(-K // 4)                   # K split four ways (the skinny kernel's waves; a split-K form): forward partials, added last
    parts = [_accumulate(a[:, i:i + q], b[:, i:i + q], "step32") for i in range(0, K, q)]
    return ((parts[0] + parts[1]) + parts[2] + parts[3]) if len(parts) == 4 else sum(parts[1:], parts[0])


class Emulator:
    """rt_conv_gemm / rt_conv_wgrad with fp32 accumulation in one of ORDERS and the epilogue of csrc/rt_gemm_common.h in fp32"""

    def __init__(self, order):
        self.order = order

    def gemm(self, spec):
        e = spec["epi"]
        A = G.gather(spec["src"], spec["geom"], spec["transposed"], spec["dil"])
        N = spec["geom"][6]
        v = _accumulate(A, spec["wgt"].reshape(N, -1), self.order)
        M = v.shape[0]
        f = lambda t: t.float()      # noqa: E731
        out = {}
        if e.get("bias") is not None:
            v = v + f(e["bias"])
        out["out_preact"] = v.bfloat16().double()

        def add_res(v):
            if e.get("res_f32") is not None:
                v = v + f(e["res_f32"])
            if e.get("res_bf16") is not None:
                v = v + f(e["res_bf16"])
            return v
        if e["res_first"]:
            v = add_res(v)
        if e["act"] == G.ACT_RELU:
            v = v.clamp(min=0)
        elif e["act"] == G.ACT_GELU:
            v = G.gelu_f32(v)
        elif e["act"] == G.ACT_TANH:
            v = torch.tanh(v)
        if e.get("drop_p", 0) > 0:
            p = np.float32(e["drop_p"])
            ks = np.float32(1.0) / (np.float32(1.0) - p)
            keep = G.keep_mask(M, N, e["drop_p"], e["drop_seed"], e["drop_shift"], e["seed_dev"])
            v = torch.where(keep, v * float(ks), torch.zeros(()))
        if not e["res_first"]:
            v = add_res(v)
        if e.get("gate") is not None:
            v = torch.where(e["gate"] > 0, v * float(np.float32(e["gate_scale"])), torch.zeros(()))
        if e.get("preact") is not None:
            v = v * G.gelu_grad_f32(e["preact"])
        if e.get("dtanh") is not None:
            t = f(e["dtanh"])
            v = v * (1.0 - t * t)
        out["out_f32"], out["out_bf16"] = v.double(), v.bfloat16().double()
        for k in ("out_f32", "out_bf16"):
            if k not in spec["stores"]:
                del out[k]
        if e.get("acc2") is not None:
            out["acc2"] = (f(e["acc2"]) + v).double()
        return out

    def wgrad(self, spec):
        N = spec["geom"][6]
        A = G.gather(spec["x"], spec["geom"], False, spec["dil"])
        dy = spec["dy"].reshape(-1, N)
        M = dy.shape[0]
        if self.order == "ksplit4":      # split-M partials, summed last
            S = max(spec["splits"], 2)
            q = -(-M // S)
            parts = [_accumulate(dy[i:i + q].t(), A[i:i + q].t(), "step32") for i in range(0, M, q)]
            a = sum(parts[1:], parts[0])
            db = sum((dy[i:i + q].float().sum(0) for i in range(q, M, q)), dy[:q].float().sum(0))
        else:
            a = _accumulate(dy.t(), A.t(), self.order)
            db = dy.float().sum(0) if self.order != "reversed" else dy.flip(0).float().sum(0)
        if spec["scale"] is not None:
            a = a * spec["scale"].float()[:, None]
        old = torch.zeros_like(a) if spec["overwrite"] else spec["dw_before"].float()
        dw = old + a
        d = a * (old + old + a)                                  # rt_wg_commit's increment
        out = dict(dw=dw.double(), g16=dw.bfloat16().double(), sq=float(d.sum()))
        if spec["dbias_before"] is not None:
            out["dbias"] = (spec["dbias_before"].float() + db).double()
        return out


# ------------------------------------------------------------------------------------------------ 1. the reference against autograd
def _autograd(name, Ci, Co, seed=0):
    if name in G.W2_CASES:              # the second generation's table: its own sizes, small channel counts here
        B, H, W, _, _, k, s, p, dil = G.W2_CASES[name]
        geom = (B, H, W, Ci, (H + 2 * p - dil * (k - 1) - 1) // s + 1, (W + 2 * p - dil * (k - 1) - 1) // s + 1, Co, k, k, s, p)
    else:
        geom, dil = G.conv_geom(name, Ci, Co)
    B, H, W, _, Ho, Wo, _, k, _, s, p = geom
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt, b, stride=s, padding=p, dilation=dil)
    assert y.shape[-2:] == (Ho, Wo)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()      # noqa: E731
    return geom, dil, nhwc(x), nhwc(wt), b, nhwc(y), nhwc(dy), nhwc(x.grad), nhwc(wt.grad), wt.detach()


def _close(a, b):
    return float((a - b.reshape(a.shape)).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize("name", list(G.GATHERS) + [n for n, c in G.W2_CASES.items() if c[1] > 1])
def test_reference_against_float64_autograd(name):
    geom, dil, x, w, b, y, dy, dx, dw, wt = _autograd(name, 8, 12)
    Co, Ci = geom[6], geom[3]
    assert _close(G.conv_gemm_ref(x, w, geom, dil=dil, bias=b).out, y.reshape(-1, Co))
    w_t = wt.permute(1, 2, 3, 0).contiguous()                          # [Ci][kh][kw][Co]: the backward-data operand
    assert _close(G.conv_gemm_ref(dy, w_t, G.transposed_geom(geom), transposed=True, dil=dil).out, dx.reshape(-1, Ci))
    r = G.conv_wgrad_ref(dy, x, geom, dil=dil)
    assert _close(r.dw, dw.reshape(Co, -1)) and _close(r.dbias, dy.sum((0, 1, 2)))
    sc, before = torch.arange(1.0, Co + 1, dtype=torch.float64), torch.ones(Co, dw[0].numel(), dtype=torch.float64)
    r2 = G.conv_wgrad_ref(dy, x, geom, dil=dil, scale=sc, dw_before=before)
    assert _close(r2.dw, before + sc[:, None] * r.dw) and abs(r2.sq - float((r2.dw ** 2).sum() - before.numel())) < 1e-9 * abs(r2.sq)
    assert _close(G.conv_wgrad_ref(dy, x, geom, dil=dil, scale=sc, dw_before=before, overwrite=True).dw, sc[:, None] * r.dw)


def test_epilogue_order_and_bound_against_plain_expressions():
    g = torch.Generator().manual_seed(1)
    M, K, N = 9, 64, 8
    s = gemm_spec("randn", linear_geom(M, K, N), g)
    x, w, b = s["src"].reshape(M, K), s["wgt"].reshape(N, K), s["epi"]["bias"]
    lin = x @ w.t() + b
    rn = lambda: torch.randn(M, N, generator=g, dtype=torch.float64)      # noqa: E731
    rf, rb, gate, pre, t, acc = rn(), rn(), rn(), rn(), torch.tanh(rn()), rn()
    ref = G.conv_gemm_ref(x, w, s["geom"], bias=b)
    assert torch.equal(ref.bound_preact, pbound(x, w, b)) and _close(ref.out_preact, lin)
    keep = G.keep_mask(M, N, 0.25, 77, 1)
    full = G.conv_gemm_ref(x, w, s["geom"], bias=b, res_f32=rf, res_bf16=rb, gate=gate, gate_scale=1.25, preact=pre, dtanh=t, act=G.ACT_GELU,
                           drop_p=0.25, drop_seed=77, drop_shift=1, acc2=acc)
    u = pre.clone().requires_grad_(True)
    F.gelu(u).sum().backward()
    want = (F.gelu(lin) * keep / 0.75 + rf + rb) * (gate > 0) * 1.25 * u.grad * (1 - t * t)
    assert _close(full.out, want) and _close(full.acc2, acc + want) and _close(full.out_preact, lin)
    first = G.conv_gemm_ref(x, w, s["geom"], bias=b, res_f32=rf, res_bf16=rb, res_first=True, act=G.ACT_RELU, drop_p=0.25, drop_seed=77)
    assert _close(first.out, torch.relu(lin + rf + rb) * G.keep_mask(M, N, 0.25, 77) / 0.75)
    assert _close(G.conv_gemm_ref(x, w, s["geom"], bias=b, act=G.ACT_TANH).out, torch.tanh(lin))


# ------------------------------------------------------------------------------------------------ 2. dropout decisions
@pytest.mark.parametrize("p,seed,shift", [(0.1, 1234, 0), (0.5, G.DROP_SEED, 2), (0.5, G.DROP_SEED, 5), (0.3, 0xFFFFFFFF, 0)])
def test_dropout_decisions_against_hash_keep(p, seed, shift):
    M, N = 37, 72
    idx = np.arange(M * N, dtype=np.uint64) >> np.uint64(shift)
    assert np.array_equal(G.keep_mask(M, N, p, seed, shift).numpy().reshape(-1), hash_keep(seed, idx, p))
    # seed_dev: the site seed is rt_hash32(*seed_dev, drop_seed) = the hash with `seed` := *seed_dev at index drop_seed
    site = int(G.hash32(G.SEED_DEV, np.array([seed], dtype=np.uint64))[0])
    assert np.array_equal(G.keep_mask(M, N, p, seed, shift, G.SEED_DEV).numpy().reshape(-1), hash_keep(site, idx, p))
    assert site != seed


# ------------------------------------------------------------------------------------------------ 3. activation constants
def test_activation_error_constants_are_the_measured_ones():
    m = G.measure_act_err()
    print("\n[activation error, fp32 expression vs float64, in its unit] " + "  ".join(f"{k}={v:.3f}" for k, v in m.items()))
    for k, v in m.items():
        assert v <= G.ACT_MEASURED[k] <= 1.05 * v + 0.01, (k, v)
        assert G.ACT_ERR[k] == 2.0 * G.ACT_MEASURED[k]


# ------------------------------------------------------------------------------------------------ 4. the bounds on the emulator
def tile_specs(hint, kinds):
    """every (case, operand set) of a tile form: (tag, spec, exact)"""
    for (M, K, N), kind in itertools.product(G.tile_form_cases(hint), kinds):
        if K == 2304 and kind not in ("ints", "randn"):
            continue
        g = torch.Generator().manual_seed(hint * 131 + M + K + N)
        yield f"hint {hint} {M}x{K}x{N} {kind}", gemm_spec(kind, linear_geom(M, K, N), g, hint=hint), kind == "ints"


def gather_specs(hint, kinds):
    """every gather of gemm_ref.GATHERS the form takes, forward and transposed, channels 64 -> 128 and 128 -> 64"""
    for i, name in enumerate(G.GATHERS):
        Ci, Co = (64, 128) if i % 2 == 0 else (128, 64)
        geom, dil = G.conv_geom(name, Ci, Co)
        for kind, tr in itertools.product(kinds, (False, True)):
            g = torch.Generator().manual_seed(hint * 17 + i)
            gm = G.transposed_geom(geom) if tr else geom
            yield f"hint {hint} {name} {'transposed' if tr else 'forward'} {kind}", gemm_spec(kind, gm, g, hint=hint, transposed=tr, dil=dil), kind == "ints"


def epilogue_specs(hint, M, K, Ns, kinds):
    for combo, N, kind in itertools.product(G.EPI_COMBOS, Ns, kinds):
        if kind == "ints" and not G.EPI_COMBOS[combo]["exact"]:
            continue
        g = torch.Generator().manual_seed(hint * 7 + N + len(combo))
        spec = gemm_spec(kind, linear_geom(M, K, N), g, hint=hint, combo=combo)
        yield f"hint {hint} {M}x{K}x{N} {kind} [{combo}]", spec, kind == "ints"
        if kind == "ints":          # tier 1 also with each store alone
            for one in single_store(spec):
                yield f"hint {hint} {M}x{K}x{N} {kind} [{combo}] {one['stores'][0]} alone", one, True


def epilogue_shape(hint):
    """(M, K, Ns): one row tile and five rows, the 4-wide and the 8-wide epilogue; hint 0: the skinny route and the first tile route"""
    BM, BN, _ = G.TILES[hint]
    return BM + 5, 128, (BN + 4, BN + 8)


def wgrad_first_gen_specs(kinds):
    """first generation: every (N, SC) x M; msplit x workspace at M = 200 and 1000; overwrite on and off.  Below 256 rows variant 0 is
    the library's own first-generation choice (the default 128 x 128 DMA tile among them); at M = 1000, where variant 0 would go to
    the second generation, variant 1 pins the DMA kernels; variant 9 is the register-staged kernel"""
    for (N, SC), M, kind in itertools.product(G.WGRAD_NC, G.WGRAD_M, kinds):
        splits = G.WGRAD_SPLITS if M >= 200 else [(0, True), (3, False)]
        first = 0 if M < 256 else 1
        for j, (msplit, ws) in enumerate(splits):
            g = torch.Generator().manual_seed(N * 3 + SC + M + j)
            for variant in ((first, 9) if j == 0 else (first,)):
                ow = (j + M) % 2 == 1
                yield (f"wgrad {M}x{SC}->{N} {kind} msplit {msplit} {'workspace' if ws else 'atomics'} variant {variant} "
                       f"{'overwrite' if ow else 'accumulate'}",
                       wgrad_spec(kind, linear_geom(M, SC, N), g, msplit=msplit, workspace=ws, variant=variant, overwrite=ow), kind == "ints")


def wgrad_gather_specs(kinds):
    """the 3x3 stride 1 / stride 2 / dil 2 gathers on the DMA kernels (variant 1) and the register-staged one (9), five images: with
    msplit 3 the last split is ragged on both (10 chunks of 32 rows in splits of 4; 5 chunks of 64 in splits of 2)"""
    for i, (name, kind, variant, msplit) in enumerate(itertools.product(G.WGRAD_GATHERS, kinds, (1, 9), (0, 3))):
        geom, dil = G.conv_geom(name, 64 if i % 2 else 128, 128 if i % 2 else 64)
        geom = (5,) + geom[1:]
        g = torch.Generator().manual_seed(900 + i)
        yield (f"wgrad {name} {kind} variant {variant} msplit {msplit}",
               wgrad_spec(kind, geom, g, dil=dil, variant=variant, msplit=msplit, overwrite=bool((i // 2) % 2)), kind == "ints")


def w2_spec(name, kind, overwrite, seed=0):
    B, H, W, Ci, Co, k, s, p, d = G.W2_CASES[name]
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    g = torch.Generator().manual_seed(seed + sum(map(ord, name)))
    return wgrad_spec(kind, (B, H, W, Ci, Ho, Wo, Co, k, k, s, p), g, dil=d, overwrite=overwrite, scale=k > 1)


KINDS = ("ints",) + G.OPERAND_SETS
CPU_HINTS = (31, 285, 51)           # a 64 x 64, the 32 x 32 deep-stage and a 128 x 128 form: the emulator does not depend on the tile


def _run_all(specs, check, orders=ORDERS):
    w = Worst()
    n = 0
    for tag, spec, exact in specs:
        for order in orders:
            check(w, Emulator(order), spec, exact, f"{tag} ({order})")
            n += 1
    assert all(v <= 1.0 for v in w.values()), w
    return w, n


@pytest.mark.parametrize("hint", CPU_HINTS)
def test_bounds_hold_on_the_emulator_tile_forms(hint):
    w, n = _run_all((s for s in tile_specs(hint, KINDS) if s[1]["geom"][3] < 2304 or hint == 31), check_gemm)
    print(w.line(f"emulator, tile forms of hint {hint}, {n} runs"))


def test_bounds_hold_on_the_emulator_gathers():
    w, n = _run_all(gather_specs(31, KINDS), check_gemm, ORDERS[2:])
    print(w.line(f"emulator, gathers, {n} runs"))


def test_bounds_hold_on_the_emulator_epilogues():
    w, n = _run_all(epilogue_specs(31, *epilogue_shape(31), KINDS), check_gemm, ORDERS[:1] + ORDERS[2:])
    print(w.line(f"emulator, epilogue combinations, {n} runs"))


def test_bounds_hold_on_the_emulator_weight_gradients():
    specs = itertools.chain(wgrad_first_gen_specs(KINDS), wgrad_gather_specs(KINDS),
                            ((f"w2 {name} {kind}", w2_spec(name, kind, i % 2 == 0), kind == "ints")
                             for i, (name, kind) in enumerate(itertools.product(G.W2_CASES, KINDS))))
    w, n = _run_all((s for s in specs if " variant 9" not in s[0]), check_wgrad, ORDERS[2:])
    print(w.line(f"emulator, weight gradients, {n} runs"))


def test_bounds_hold_on_the_emulator_weight_gradients_row_by_row():
    """forward and reversed row order (one fp32 addition per row) on the smallest and the largest first-generation shape"""
    specs = [s for s in wgrad_first_gen_specs(G.OPERAND_SETS) if s[0].startswith(("wgrad 77x64->64 ", "wgrad 1000x144->132 "))
             and "msplit 0 workspace variant " in s[0] and " variant 9" not in s[0]]
    assert len(specs) == 6
    w, n = _run_all(specs, check_wgrad, ORDERS[:2])
    print(w.line(f"emulator, weight gradients row by row, {n} runs"))


class OneOff(Emulator):
    """the emulator with one element of one output off: one integer in fp32, 2^-6 of itself (of 1 below 1) in bf16"""

    def __init__(self, key):
        super().__init__("step32")
        self.key = key

    def gemm(self, spec):
        out = super().gemm(spec)
        t = out[self.key]
        t[-1, -1] += 1.0 if self.key == "out_f32" else 2.0 ** -6 * max(abs(float(t[-1, -1])), 1.0)
        return out


@pytest.mark.parametrize("kind", ["ints", "randn"])
@pytest.mark.parametrize("key", ["out_f32", "out_bf16"])
def test_a_wrong_element_is_noticed(kind, key):
    """the checks themselves: the last element off fails, tier 1 and tier 2"""
    spec = gemm_spec(kind, linear_geom(65, 64, 68), torch.Generator().manual_seed(3))
    check_gemm(Worst(), Emulator("step32"), spec, kind == "ints", "probe")
    with pytest.raises(AssertionError, match=key):
        check_gemm(Worst(), OneOff(key), spec, kind == "ints", "probe")
