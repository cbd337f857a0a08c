"""Plain float64 definitions of the optimizer step of csrc/rt_optim.hip -- rt_sqnorm / rt_sqnorm_bf16, the clip, AdamW (rt_adamw_flat,
rt_adamw_chunks, rt_adamw_mat with the bf16 operands it emits) and rt_sgd_flat -- with the element-wise error bounds
tests/test_optim_ref_cpu.py proves usable on an fp32 emulation and tests/test_optim_fp64_gpu.py holds the kernels to.  CPU only.

Every constant the descriptor carries as fp32 (beta1, beta2, eps, lr, wd, grad_scale, max_norm, the clip's 1e-6) enters as the float64
value of that fp32 number (f32()): the reference describes the arithmetic asked of the kernel, not the decimal literal.

    total = sqrt(sq) grad_scale;  coef = min(1, max_norm / (total + 1e-6)) if max_norm > 0 else 1;  gs = grad_scale coef
    m' = b1 m + (1 - b1) g gs;    v' = b2 v + (1 - b2) (g gs)^2
    p' = p (1 - lr wd) - lr / (1 - b1^step) m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    SGD:  g' = g gs + wd p;  m' = momentum m + g';  p' = p - lr m'

Bounds.  u = 2^-24 is the unit roundoff of fp32 (half an ulp, relative): one u per fp32 rounding of the WIDEST of the three forms of
adam_elem -- the plain text with nothing fused; a fused multiply-add only removes roundings.  All bounds are absolute and stated
against sums of absolute values, never relative to a result: b1 m + (1 - b1) g gs cancels.  First order in u; the second-order terms
are below 2^-12 of them here, and every bound is multiplied by 1 + 2^-10 (SECOND_ORDER) for them.

  gs        clip engaged: sqrtf (S u), x grad_scale (u), + 1e-6 (u), the division (D u), grad_scale x coef (u):  d_gs = (S + D + 3) u,
            relative.  Not engaged or max_norm <= 0: coef is exactly 1 and gs = grad_scale exactly, d_gs = 0.
  gnorm_out sqrtf and one product: (S + 1) u total
  m'        A = |b1 m|, B = |(1 - b1) g gs|.  b1 m rounds once and meets the sum's rounding: 2 u A.  On B: g gs (u, and d_gs),
            1 - b1 (u), their product (u), the sum (u):  E_m = 2 u A + (4 u + d_gs) B
  v'        C = b2 v, D = (1 - b2) (g gs)^2, both >= 0.  2 u C as above; on D: g gs twice (2 u + 2 d_gs), 1 - b2 (u), two products
            (2 u), the sum (u):  E_v = 2 u C + (6 u + 2 d_gs) D
  bc        pw = powf(b, step) is off by P u b^step, bc = 1 - pw rounds once: |bc err| <= P u b^step + u bc, that is
            d_bc = u (1 + P b^step / (1 - b^step)) relative -- the amplification b^step / (1 - b^step) is 999 for beta2 at step 1
  lr / bc1  d_c1 = d_bc1 + D u
  isb2      rsqrtf(bc2): d_isb2 = d_bc2 / 2 + R u
  denom     den = sqrt(v') isb2 + eps:  E_den = isb2 E_v / (2 sqrt v') + (S u + d_isb2 + u) sqrt(v') isb2 + u den
  p'        q = m' / den:  E_q = E_m / den + |m'| E_den / den^2 + D u |q|;  upd = (lr / bc1) q:  E_upd = (lr / bc1) E_q + (d_c1 + u) |upd|
            the decay factor: lr wd (u lr wd), 1 - lr wd (u), its product with p (u); the final subtraction u |p'|:
            E_p = E_upd + (2 + lr wd) u |p| + u |p'|
  SGD       g' = fma(g, gs, wd p): E_g = u |wd p| + d_gs |g gs| + u |g'|;  m' = fma(b1, m, g'): E_m = E_g + u |m'|;
            p' = fma(-lr, m', p): E_p = lr E_m + u |p'|
  norm      all summands are positive, so the bound is (1 + u)^chain - 1 of the sum, chain = the longest run of roundings one
            summand passes through (sqnorm_chain)

S, D, R, P: the error of sqrtf, the division, rsqrtf and powf in units of u.  MEASURED on the host's fp32 functions against float64
(measure_math_err; tests/test_optim_ref_cpu.py re-measures and compares) and doubled for the device's math library (MATH_FACTOR), as
gemm_ref.ACT_MEASURED is.  Nothing here is taken from a kernel's output.
"""
import math
import types

import numpy as np
import torch

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
TINY = 2.0 ** -126                   # a result below it may be flushed or lose bits: absolute slack of powf
# worst relative error of the host's fp32 function against float64, in units of u (0.5 ulp of a value just above a power of two is 1 u):
#   sqrt   1.05  (the vectorised sqrt)       div    1.00  correctly rounded
#   rsqrt  1.50  1 / sqrt, two roundings    pow    1.00  over beta in {0.5 .. 0.9999}, steps 1 .. 200000 (results >= 2^-126)
MATH_MEASURED = {"sqrt": 1.05, "div": 1.00, "rsqrt": 1.50, "pow": 1.00}
MATH_FACTOR = 2.0
MATH_ERR = {k: MATH_FACTOR * v for k, v in MATH_MEASURED.items()}
STEPS = (1, 2, 7, 1000, 30000, 120000)           # at 120000 powf(0.999, step) = 7e-53 underflows to 0 in fp32 (2^-149 = 1.4e-45)
OPERAND_SETS = ("randn", "cancel", "eps", "wide", "sharp")


def f32(x):
    """the float64 value of the fp32 number nearest to x"""
    return float(np.float32(x))


def r32(t):
    """a float64 tensor rounded to fp32 values"""
    return t.float().double()


def measure_math_err():
    """worst relative error, in units of u, of the host's fp32 sqrt, division, rsqrt and pow against float64"""
    g = torch.Generator().manual_seed(3)
    x = r32(torch.cat([torch.logspace(-60, 40, 200001, base=2.0, dtype=torch.float64), torch.rand(200000, generator=g, dtype=torch.float64) + 1e-3]))
    y = r32(torch.rand(x.numel(), generator=g, dtype=torch.float64) + 0.25)
    out = {"sqrt": float(((x.float().sqrt().double() - x.sqrt()).abs() / x.sqrt()).max() / U),
           "rsqrt": float(((x.float().rsqrt().double() - x.rsqrt()).abs() / x.rsqrt()).max() / U),
           "div": float((((x.float() / y.float()).double() - x / y).abs() / (x / y)).max() / U)}
    steps = torch.cat([torch.arange(1, 4097), torch.randint(4097, 200001, (20000,), generator=g)]).double()
    worst = 0.0
    for b in (0.9, 0.999, 0.5, 0.8, 0.95, 0.99, 0.9999):
        b32 = torch.tensor(f32(b), dtype=torch.float64)
        ref = b32 ** steps
        got = torch.pow(b32.float(), steps.float()).double()
        ok = ref >= TINY
        worst = max(worst, float(((got - ref).abs() / ref)[ok].max() / U))
    out["pow"] = worst
    return out


# ------------------------------------------------------------------------------------------------ the norm and the clip
def sqnorm_ref(g):
    """sum g^2 of an fp32 or bf16 buffer (any tensor whose values are that buffer's)"""
    return float((g.double() ** 2).sum())


def sqnorm_chain(n, bf16):
    """The longest run of fp32 roundings between one g^2 and the word rt_sqnorm / rt_sqnorm_bf16 leaves.  The host launches
    blocks = clamp(ceil((n / W) / 256), 1, 2048) workgroups of 256 threads over nv = n / W vectors of W = 4 (fp32) or 8 (bf16)
    elements, so a thread runs iters = ceil(nv / (256 blocks)) vector iterations.  A summand is squared (1); fp32 adds the four squares
    of a vector left to right (3) and then the vector to the thread's sum (1 per iteration), bf16 adds its eight squares to the
    thread's sum one by one (8 per iteration); the ragged tail adds at most one element per thread (1); the wave's butterfly (6), the
    four wave sums of the workgroup (4), and one atomic addition per workgroup in any order (blocks)."""
    W = 8 if bf16 else 4
    nv = n // W
    blocks = min(max((nv + 255) // 256, 1), 2048)
    iters = -(-nv // (256 * blocks))
    return 1 + (0 if bf16 else 3) + iters * (8 if bf16 else 1) + 1 + 6 + 4 + blocks


def sqnorm_bound(g, bf16):
    return ((1.0 + U) ** sqnorm_chain(g.numel(), bf16) - 1.0) * sqnorm_ref(g)


def clip_ref(sq, grad_scale=1.0, max_norm=0.0, word=True):
    """total, gs = grad_scale coef, and the bounds: `sq` is the fp32 word the kernel reads (None: the kernel reads 0; word=False: a
    float64 squared norm taken as it is)"""
    gsc, mx = f32(grad_scale), f32(max_norm)
    total = math.sqrt((f32(sq) if word else sq) if sq is not None else 0.0) * gsc
    S, D = MATH_ERR["sqrt"], MATH_ERR["div"]
    raw = mx / (total + f32(1e-6)) if mx > 0 else math.inf
    engaged = raw < 1.0 + 1e-5                       # within reach of 1: the kernel's quotient may fall on either side of the min
    coef = min(1.0, raw)
    return types.SimpleNamespace(total=total, bound_total=(S + 1) * U * total * SECOND_ORDER, coef=coef, gs=gsc * coef,
                                 d_gs=(S + D + 3) * U if engaged else 0.0, engaged=engaged)


# ------------------------------------------------------------------------------------------------ the updates
def range_values(n, ranges):
    """lr and wd per element: the last matching range wins, no range gives 0"""
    lr, wd = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for b, e, l, w in ranges:
        lr[b:e] = f32(l); wd[b:e] = f32(w)
    return lr, wd


def bias_corrections(step, beta1, beta2):
    """bc1, 1 / sqrt(bc2) and the relative bounds d_c1 of lr / bc1 and d_isb2 of rsqrtf(bc2)"""
    P, D, R = MATH_ERR["pow"], MATH_ERR["div"], MATH_ERR["rsqrt"]
    out = []
    for b in (f32(beta1), f32(beta2)):
        pw = b ** step
        bc = 1.0 - pw
        out.append((bc, U + (P * U * pw + (TINY if pw > 0 else 0.0)) / bc))
    (bc1, d1), (bc2, d2) = out
    return types.SimpleNamespace(bc1=bc1, isb2=1.0 / math.sqrt(bc2), d_c1=d1 + D * U, d_isb2=d2 / 2 + R * U)


def adamw_ref(p, g, m, v, ranges, step, *, gs=1.0, d_gs=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """float64 p', m', v' of one AdamW step over whole buffers (float64 tensors of fp32 / bf16 values) and their bounds"""
    b1, b2, ep = f32(beta1), f32(beta2), f32(eps)
    S, D = MATH_ERR["sqrt"], MATH_ERR["div"]
    lr, wd = range_values(p.numel(), ranges)
    c = bias_corrections(step, beta1, beta2)
    gg = g * gs
    A, B = (b1 * m).abs(), ((1 - b1) * gg).abs()
    m1 = b1 * m + (1 - b1) * gg
    E_m = 2 * U * A + (4 * U + d_gs) * B
    C, Dv = b2 * v, (1 - b2) * gg * gg
    v1 = C + Dv
    E_v = 2 * U * C + (6 * U + 2 * d_gs) * Dv
    sv = v1.sqrt()
    den = sv * c.isb2 + ep
    E_den = c.isb2 * torch.where(sv > 0, E_v / (2 * sv).clamp(min=1e-300), E_v.sqrt()) + (S * U + c.d_isb2 + U) * sv * c.isb2 + U * den
    q = m1 / den
    E_q = E_m / den + m1.abs() * E_den / (den * den) + D * U * q.abs()
    c1 = lr / c.bc1
    upd = c1 * q
    E_upd = c1 * E_q + (c.d_c1 + U) * upd.abs()
    p1 = p * (1 - lr * wd) - upd
    E_p = E_upd + (2 + lr * wd) * U * p.abs() + U * p1.abs()
    return types.SimpleNamespace(p=p1, m=m1, v=v1, upd=upd, bound_p=E_p * SECOND_ORDER, bound_m=E_m * SECOND_ORDER, bound_v=E_v * SECOND_ORDER)


def sgd_ref(p, g, m, ranges, *, gs=1.0, d_gs=0.0, momentum=0.9):
    """torch.optim.SGD(momentum, weight_decay; dampening 0, no Nesterov) as the comment above sgd_elem states it:
    g' = gs g + wd p;  buf = momentum buf + g';  p -= lr buf"""
    b1 = f32(momentum)
    lr, wd = range_values(p.numel(), ranges)
    g1 = g * gs + wd * p
    E_g = U * (wd * p).abs() + d_gs * (g * gs).abs() + U * g1.abs()
    m1 = b1 * m + g1
    E_m = E_g + U * m1.abs()
    p1 = p - lr * m1
    E_p = lr * E_m + U * p1.abs()
    return types.SimpleNamespace(p=p1, m=m1, bound_p=E_p * SECOND_ORDER, bound_m=E_m * SECOND_ORDER)


def operands_ref(p1, N, T, C, scale=None):
    """the bf16 image W [N][T][C] of p' scale[n] and its transpose WT [C][T][N], as float64, of a p' of fp32 values.  The kernel
    multiplies in fp32 and rounds the product to bf16: the image is taken the same way and has one legal value per element."""
    w = p1.reshape(N, T, C).float()
    if scale is not None:
        w = w * scale.float().view(N, 1, 1)
    w = w.to(torch.bfloat16).double()
    return w, w.permute(2, 1, 0).contiguous()


def operands_exact(p1, bound_p, N, T, C, scale=None):
    """p' scale[n] of the float64 p', unrounded, [N][T][C] and [C][T][N], and the bound of its bf16 store: the bound of p' through
    the fp32 product (u) plus half a bf16 ulp, 2^-8 |ref|"""
    s = torch.ones(N, dtype=torch.float64) if scale is None else scale.double()
    w = p1.reshape(N, T, C) * s.view(N, 1, 1)
    b = (bound_p.reshape(N, T, C) * s.abs().view(N, 1, 1) + (U if scale is not None else 0.0) * w.abs()) * (1 + 2.0 ** -8) + 2.0 ** -8 * w.abs()
    tr = lambda t: t.permute(2, 1, 0).contiguous()          # noqa: E731
    return w, tr(w), b, tr(b)


# ------------------------------------------------------------------------------------------------ operands
def operands(kind, n, g, *, bf16_grads=False, gs_of=None, beta1=0.9):
    """p, grad, m, v (float64 tensors of fp32 values; the gradient of bf16 values when bf16_grads) of one operand set:
    randn   p ~ N(0, 1), g ~ 0.01 N, m ~ 0.01 N, v ~ U(0, 1e-3)
    cancel  randn with m chosen so that b1 m and (1 - b1) g gs agree to 2^-6 with opposite signs (gs_of(grad): the clip's factor)
    eps     g, m ~ 1e-8 N, v ~ 1e-16 U: eps = 1e-8 is a first-order part of the denominator
    wide    |p|, |g|, |m|, v = 2^U(-20, 8) with random signs
    sharp   randn with |p| <= 2^-14: an ulp of p lies below the rounding of the update itself"""
    rn = lambda s=1.0: torch.randn(n, generator=g, dtype=torch.float64) * s          # noqa: E731
    ru = lambda: torch.rand(n, generator=g, dtype=torch.float64)                      # noqa: E731
    if kind == "wide":
        mag = lambda: 2.0 ** (ru() * 28 - 20) * torch.where(ru() < 0.5, -1.0, 1.0)  # noqa: E731
        p, gr, m, v = mag(), mag(), mag(), mag().abs()
    elif kind == "eps":
        p, gr, m, v = rn(), rn(1e-8), rn(1e-8), ru() * 1e-16
    else:
        p, gr, m, v = rn(), rn(0.01), rn(0.01), ru() * 1e-3
        if kind == "sharp":
            p = (ru() * 2 - 1) * 2.0 ** -14
    gr = gr.bfloat16().double() if bf16_grads else r32(gr)
    if kind == "cancel":
        b1 = f32(beta1)
        m = -(1 - b1) * gr * gs_of(gr) / b1 * (1 + 2.0 ** -6 * rn())
    return r32(p), gr, r32(m), r32(v)
