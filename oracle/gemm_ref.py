"""Plain float64 definitions of rt_conv_gemm and rt_conv_wgrad (include/reftr_hip.h), with the element-wise error bounds and the
case tables tests/test_gemm_ref_cpu.py and tests/test_gemm_fp64_gpu.py share.  Everything here runs on the CPU.

The gathers are written from the header's two formulas, the epilogue in the order of csrc/rt_gemm_common.h:

    +bias -> store preact -> [+res if res_first] -> act -> dropout -> [+res] -> *gate -> *gelu'(preact) -> *(1 - dtanh^2)

Bounds (u = 2^-23, products of two bf16 values are exact in fp32):
  fp32 product + bias + residuals   (K + 2) u (|x| |w|^T + |bias| + |res|): K - 1 additions, the bias and two residual additions
  ... through the epilogue          1-Lipschitz terms (ReLU, the gate's 0 / 1) leave it, factors (1 / (1 - p), gate_scale, gelu',
                                    1 - t^2) multiply it; each factor rounds once more: MUL_ROUNDINGS u |result| in all
  GELU, tanh, gelu'                 Lipschitz constant times the bound + the error of the fp32 expression itself (ACT_ERR below)
  bf16 stores                       + 2^-8 |ref|
  weight gradients                  (M + S + 2) u |scale| sum |dy x| + u |dw before|, S = the additions of the split reduction
  sqacc                             see sq_bound
"""
import math
import types

import numpy as np
import torch

U32, U16 = 2.0 ** -23, 2.0 ** -8
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3
MUL_ROUNDINGS = 6          # keep scale, gate_scale, gelu' product, t * t, 1 - t^2, its product: one rounding each

# Error of the fp32 expressions of csrc/rt_common.h (rt_gelu, rt_gelu_grad) and of tanhf against float64, in the unit each one scales
# with, over |x| <= ACT_RANGE: MEASURED on the CPU by measure_act_err() (tests/test_gemm_ref_cpu.py re-measures and compares), times
# ACT_FACTOR for the device's math library (erff, tanhf, __expf are not the host's).  Not taken from any kernel's output.
#   gelu   |err| <= c u |x|              measured c = 0.86
#   tanh   |err| <= c u |tanh x|         measured c = 0.53
#   gelu'  |err| <= c u (1 + |x|)        measured c = 0.55
ACT_RANGE = 128.0
ACT_MEASURED = {"gelu": 0.86, "tanh": 0.53, "gelu_grad": 0.55}
ACT_FACTOR = 2.0
ACT_ERR = {k: ACT_FACTOR * v for k, v in ACT_MEASURED.items()}
GELU_LIP = 1.13            # max |gelu'| = 1.1289


# ------------------------------------------------------------------------------------------------ float64 pieces
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_f32(x):
    """rt_gelu, every operation in fp32"""
    x = x.float()
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def gelu_grad_f32(x):
    """rt_gelu_grad, every operation in fp32"""
    x = x.float()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
    pdf = 0.39894228040143267794 * torch.exp(-0.5 * x * x)
    return cdf + x * pdf


def measure_act_err():
    """worst error of the fp32 expressions against float64 over |x| <= ACT_RANGE, in the units of ACT_ERR"""
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.linspace(-ACT_RANGE, ACT_RANGE, 400001, dtype=torch.float64), 8 * torch.randn(400000, generator=g).double(),
                   torch.logspace(-20, 7, 100000, base=2.0, dtype=torch.float64), -torch.logspace(-20, 7, 100000, base=2.0, dtype=torch.float64)])
    x = x.float().double()
    x = x[x != 0]
    t64 = torch.tanh(x)
    return {"gelu": float(((gelu_f32(x).double() - gelu(x)).abs() / (U32 * x.abs())).max()),
            "tanh": float(((torch.tanh(x.float()).double() - t64).abs() / (U32 * t64.abs())).max()),
            "gelu_grad": float(((gelu_grad_f32(x).double() - gelu_grad(x)).abs() / (U32 * (1 + x.abs()))).max())}


def hash32(seed, idx):
    """rt_hash32 (csrc/rt_common.h) on numpy uint64 arrays"""
    m = np.uint64(0xFFFFFFFF)
    x = ((np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1)) & m) ^ np.uint64(seed)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def keep_mask(M, N, drop_p, drop_seed, drop_shift=0, seed_dev=None):
    """the epilogue's dropout decisions [M, N]: rt_hash32(site seed, (m N + n) >> drop_shift) >= rt_drop_thresh(p)"""
    site = int(hash32(seed_dev, np.uint64(drop_seed))) if seed_dev is not None else drop_seed
    idx = np.arange(M * N, dtype=np.uint64) >> np.uint64(drop_shift)
    thresh = np.uint64(int(float(np.float32(drop_p)) * 4294967296.0))
    return torch.from_numpy((hash32(site, idx) >= thresh).reshape(M, N))


def gather(src, geom, transposed=False, dil=1):
    """The implicit GEMM's left operand [M, KH KW SC] of src [B, SH, SW, SC]:
    forward     source pixel (y stride - pad + kh dil, x stride - pad + kw dil)
    transposed  source pixel ((y + pad - kh dil) / stride, (x + pad - kw dil) / stride) where divisible
    taps outside the source read zero."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    dil = max(int(dil), 1)

    def axis(D, S, Kn):
        d, k = torch.arange(D)[:, None], torch.arange(Kn)[None, :]
        if not transposed:
            s = d * stride - pad + k * dil
            ok = s >= 0
        else:
            n = d + pad - k * dil
            ok = (n >= 0) & (n % stride == 0)
            s = torch.div(n, stride, rounding_mode="floor")
        ok = ok & (s < S)
        return s.clamp(0, S - 1), ok
    sy, oky = axis(DH, SH, KH)
    sx, okx = axis(DW, SW, KW)
    src = src.reshape(B, SH, SW, SC)
    a = src[:, sy][:, :, :, sx]                                      # [B, DH, KH, DW, KW, SC]
    a = a * (oky[None, :, :, None, None, None] & okx[None, None, None, :, :, None])
    return a.permute(0, 1, 3, 2, 4, 5).reshape(B * DH * DW, KH * KW * SC)


def conv_gemm_ref(src, wgt, geom, *, transposed=False, dil=1, bias=None, res_f32=None, res_bf16=None, gate=None, gate_scale=1.0,
                  preact=None, dtanh=None, res_first=False, act=ACT_NONE, drop_p=0.0, drop_seed=0, drop_shift=0, seed_dev=None,
                  acc2=None):
    """float64 out [M, N], out_preact and acc2 (its value after the call) of one rt_conv_gemm; every tensor argument float64.
    Also the fp32 error bounds of the three: `bound`, `bound_preact`, `bound_acc2` (bf16 stores add U16 |ref|)."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    A = gather(src, geom, transposed, dil)
    W = wgt.reshape(N, KH * KW * SC)
    M, K = A.shape
    v = A @ W.t()
    mag = A.abs() @ W.abs().t()
    if bias is not None:
        v = v + bias
        mag = mag + bias.abs()
    pre = v.clone()
    err = (K + 2) * U32 * mag
    bound_pre = err.clone()
    res = None
    if res_f32 is not None or res_bf16 is not None:
        res = (res_f32 if res_f32 is not None else 0) + (res_bf16 if res_bf16 is not None else 0)
        res_mag = (res_f32.abs() if res_f32 is not None else 0) + (res_bf16.abs() if res_bf16 is not None else 0)
    if res is not None and res_first:
        v, err = v + res, err + (K + 2) * U32 * res_mag
    if act == ACT_RELU:
        v = v.clamp(min=0)
    elif act == ACT_GELU:
        err = GELU_LIP * err + ACT_ERR["gelu"] * U32 * (v.abs() + err)
        v = gelu(v)
    elif act == ACT_TANH:
        v = torch.tanh(v)
        err = err + ACT_ERR["tanh"] * U32 * v.abs()
    if drop_p > 0:
        ks = 1.0 / (1.0 - float(np.float32(drop_p)))
        keep = keep_mask(M, N, drop_p, drop_seed, drop_shift, seed_dev)
        v, err = torch.where(keep, v * ks, 0.0), torch.where(keep, err * ks, 0.0)
    if res is not None and not res_first:
        v, err = v + res, err + (K + 2) * U32 * res_mag
    if gate is not None:
        on = gate > 0
        v, err = torch.where(on, v * gate_scale, 0.0), torch.where(on, err * abs(gate_scale), 0.0)
    if preact is not None:
        gg = gelu_grad(preact)
        err = err * gg.abs() + v.abs() * ACT_ERR["gelu_grad"] * U32 * (1 + preact.abs())
        v = v * gg
    if dtanh is not None:
        f = 1.0 - dtanh * dtanh
        v, err = v * f, err * f.abs() + 2 * U32 * v.abs()           # t * t and 1 - t^2 round once each, relative to 1 >= |f|
    err = err + MUL_ROUNDINGS * U32 * v.abs()
    out = types.SimpleNamespace(out=v, out_preact=pre, bound=err, bound_preact=bound_pre, acc2=None, bound_acc2=None, M=M, N=N, K=K)
    if acc2 is not None:
        out.acc2 = acc2 + v
        out.bound_acc2 = err + U32 * out.acc2.abs()
    return out


def conv_wgrad_ref(dy, x, geom, *, dw_before=None, scale=None, overwrite=False, dil=1, dbias_before=None, splits=1):
    """float64 dw [N, KH KW SC], dbias, the bf16 twin's exact value (= dw: the twin is its rounding) and the sqacc increment
    |dw after|^2 - |dw before|^2 of one rt_conv_wgrad, with their fp32 bounds.  `splits`: S of the bound."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    A = gather(x, geom, False, dil)
    M = A.shape[0]
    dy = dy.reshape(M, N)
    prod, mag = dy.t() @ A, dy.abs().t() @ A.abs()
    if scale is not None:
        prod, mag = prod * scale[:, None], mag * scale.abs()[:, None]
    before = torch.zeros_like(prod) if (overwrite or dw_before is None) else dw_before.reshape(prod.shape)
    dw = before + prod
    bound = (M + splits + 2) * U32 * mag + U32 * before.abs()
    db0 = dbias_before if dbias_before is not None else torch.zeros(N, dtype=torch.float64)
    dbias = db0 + dy.sum(0)
    bound_db = (M + splits + 2) * U32 * dy.abs().sum(0) + U32 * db0.abs()
    return types.SimpleNamespace(dw=dw, dbias=dbias, g16=dw, sq=float((dw * dw).sum() - (before * before).sum()), bound=bound,
                                 bound_dbias=bound_db, before=before, M=M)


def sq_bound(after, before, slots=256):
    """|after|^2 - |before|^2 as the kernels add it up, against the same sum in float64 OVER THE KERNEL'S OWN dw: n = N K terms, each
    a product pair rounded in fp32 (4 roundings: the square or a (2 old + a), the re-rounded sum old + a twice), added in any order
    (n - 1 additions) into at most `slots` accumulator words that are then added up: (n + slots + 4) u sum (after^2 + before^2)"""
    n = after.numel()
    return (n + slots + 4) * U32 * float((after * after).sum() + (before * before).sum())


# ------------------------------------------------------------------------------------------------ operands
def bf(t):
    return t.bfloat16().double()


def ints(shape, g, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


OPERAND_SETS = ("randn", "cancel", "x16")


def operand_pair(kind, a_shape, b_shape, axis_a, axis_b, fan, g):
    """Two operands contracted over axis_a of a / axis_b of b (both of even length where `cancel` is to bite):
    ints    integers -3 .. 3 (tier 1)
    randn   bf16(randn), bf16(randn / sqrt(fan))
    cancel  the second half of the contraction axis repeats b and negates a up to a 2^-6 perturbation: every product sum cancels
            to about 2^-6 of sum |a b|
    x16     randn, both scaled by 16"""
    if kind == "ints":
        return ints(a_shape, g), ints(b_shape, g)
    a, b = bf(torch.randn(a_shape, generator=g)), bf(torch.randn(b_shape, generator=g) / fan ** 0.5)
    if kind == "x16":
        return a * 16, b * 16
    if kind == "cancel":
        ha, hb = a.shape[axis_a] // 2, b.shape[axis_b] // 2
        lo_a, lo_b = a.narrow(axis_a, 0, ha), b.narrow(axis_b, 0, hb)
        pert = bf(2.0 ** -6 * torch.randn(lo_a.shape, generator=g))
        a.narrow(axis_a, ha, ha).copy_(bf(pert - lo_a))
        b.narrow(axis_b, hb, hb).copy_(lo_b)
    return a, b


# ------------------------------------------------------------------------------------------------ case tables
# hint -> (BM, BN, NS) of the product library's tile forms (csrc/rt_gemm.hip, rt_gemm_pipe.hip)
TILES = {21: (128, 64, 2), 31: (64, 64, 2), 33: (64, 64, 3), 51: (128, 128, 2), 233: (64, 64, 3), 252: (128, 128, 3), 262: (256, 128, 3),
         281: (32, 32, 3), 285: (32, 32, 6)}
GATHER_HINTS = (21, 31, 33, 51, 233, 252)         # 262, 281, 285 are dense-only forms


def tile_form_cases(hint):
    """(M, K, N): M one short of a tile and two tiles + 5, N four and eight past a tile (the 4-wide and the 8-wide epilogue), K of
    one tile, as many as stages, one more; K = 2304 once"""
    BM, BN, NS = TILES[hint]
    out = [(M, K, N) for M in (BM - 1, 2 * BM + 5) for N in (BN + 4, BN + 8) for K in (64, 64 * NS, 64 * (NS + 1))]
    return out + [(2 * BM + 5, 2304, BN + 8)]


# name -> (B, SH, SW, k, stride, pad, dil); the destination size follows.  Each runs forward and transposed.
GATHERS = {
    "3x3 s1 p1": (2, 7, 9, 3, 1, 1, 1),
    "3x3 s2 p1 odd": (2, 13, 11, 3, 2, 1, 1),
    "1x1 s2": (2, 12, 13, 1, 2, 0, 1),
    "3x3 dil2 p2": (2, 9, 7, 3, 1, 2, 2),
    "3x3 dil3 p3": (2, 9, 10, 3, 1, 3, 3),
    "3x3 s1 p0": (2, 7, 9, 3, 1, 0, 1),
}


def conv_geom(name, Ci, Co):
    """forward geom (B, H, W, Ci, Ho, Wo, Co, k, k, s, p), dil"""
    B, H, W, k, s, p, d = GATHERS[name]
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    return (B, H, W, Ci, Ho, Wo, Co, k, k, s, p), d


def transposed_geom(geom):
    B, H, W, Ci, Ho, Wo, Co, k, _, s, p = geom
    return (B, Ho, Wo, Co, H, W, Ci, k, k, s, p)


# The epilogue combinations of the model's call sites (reftr_amd/models/backbone.py, net.py, reftr_transformer.py, segmentation.py).
# exact: every term stays an integer / power-of-two multiple (tier 1 runs it); the others meet GELU / tanh / gelu' (tier 2 only).
EPI_COMBOS = {
    "bottleneck tail: bias + res_bf16 first + relu": dict(bias=1, res_bf16=1, res_first=1, act=ACT_RELU, exact=1),
    "backward-data: gate + res_bf16 + res_f32": dict(gate=1, res_bf16=1, res_f32=1, exact=1),
    "in-place accumulation: gate, out_f32 is res_f32": dict(gate=1, gate_scale=2.0, res_f32=1, alias=1, exact=1),
    "bias + dropout + res_f32": dict(bias=1, drop=(0, False), res_f32=1, exact=1),
    "ffn hidden: bias + relu + dropout shift 2, seed_dev": dict(bias=1, act=ACT_RELU, drop=(2, True), exact=1),
    "one-key attention: bias + dropout shift 5, seed_dev": dict(bias=1, drop=(5, True), exact=1),
    "gated ffn backward: gate, gate_scale": dict(gate=1, gate_scale=2.0, exact=1),
    "pos gradient: acc2 beside the stores": dict(acc2=1, exact=1),
    "relu + preact store": dict(bias=1, act=ACT_RELU, out_preact=1, exact=1),
    "pooler backward: dtanh": dict(dtanh=1, exact=1),
    "gelu + preact store": dict(bias=1, act=ACT_GELU, out_preact=1, exact=0),
    "gelu backward: preact": dict(preact=1, exact=0),
    "tanh": dict(bias=1, act=ACT_TANH, exact=0),
}
DROP_SEED, SEED_DEV = 4242, 0x1234ABCD


def epilogue_tensors(combo, M, N, g, exact):
    """the float64 epilogue operands of a combination: integers (halves for dtanh) when exact, bf16 / fp32 randn otherwise"""
    c = EPI_COMBOS[combo] if isinstance(combo, str) else combo
    rn = (lambda *s: ints(s, g)) if exact else (lambda *s: torch.randn(*s, generator=g).float().double())
    rb = (lambda *s: ints(s, g)) if exact else (lambda *s: bf(torch.randn(*s, generator=g)))
    kw = dict(act=c.get("act", ACT_NONE), res_first=bool(c.get("res_first")), gate_scale=c.get("gate_scale", 1.0))
    if c.get("bias"):
        kw["bias"] = rn(N)
    if c.get("res_f32"):
        kw["res_f32"] = rn(M, N)
    if c.get("res_bf16"):
        kw["res_bf16"] = rb(M, N)
    if c.get("gate"):
        kw["gate"] = rb(M, N)
    if c.get("preact"):
        kw["preact"] = rb(M, N)
    if c.get("dtanh"):
        kw["dtanh"] = ints((M, N), g, -2, 2) / 2 if exact else bf(torch.tanh(torch.randn(M, N, generator=g)))
    if c.get("acc2"):
        kw["acc2"] = rn(M, N)
    if "drop" in c:
        shift, dev = c["drop"]
        kw.update(drop_p=0.5 if exact else 0.1, drop_seed=DROP_SEED, drop_shift=shift, seed_dev=SEED_DEV if dev else None)
    return kw, bool(c.get("out_preact")), bool(c.get("alias"))


# first-generation weight gradients: (N, SC) x M, msplit x workspace
WGRAD_NC = [(64, 64), (68, 80), (128, 64), (64, 128), (128, 128), (132, 144)]
WGRAD_M = (77, 200, 1000)
WGRAD_SPLITS = [(0, True), (1, True), (3, True), (3, False), (1000, True), (1000, False), (0, False)]       # (msplit, workspace)
WGRAD_GATHERS = ("3x3 s1 p1", "3x3 s2 p1 odd", "3x3 dil2 p2")
# second generation (rt_w2_eligible: M >= 256, N and SC >= 64 and multiples of 8, variant 0, msplit 0) at its smallest geometries:
# (B, H, W, Ci, Co, k, s, p, dil)
W2_CASES = {
    "linear 256 x 64 -> 64": (256, 1, 1, 64, 64, 1, 1, 0, 1),
    "linear 261 x 72 -> 64 (C % 16 = 8)": (261, 1, 1, 72, 64, 1, 1, 0, 1),
    "linear 300 x 136 -> 72": (300, 1, 1, 136, 72, 1, 1, 0, 1),
    "linear 600 x 264 -> 136": (600, 1, 1, 264, 136, 1, 1, 0, 1),
    "3x3 s1 p1 fused taps": (2, 12, 11, 64, 64, 3, 1, 1, 1),
    "3x3 s2 p1": (2, 23, 25, 64, 72, 3, 2, 1, 1),
    "3x3 dil2 p2": (2, 12, 11, 72, 64, 3, 1, 2, 2),
    "1x1 s2": (2, 23, 24, 64, 64, 1, 2, 0, 1),
}
