"""CPU: oracle/optim_ref.py, the float64 reference and the element-wise bounds tests/test_optim_fp64_gpu.py holds the optimizer
kernels of csrc/rt_optim.hip to.

  1. adamw_ref + clip_ref against torch.optim.AdamW on float64 parameters behind clip_grad_norm_ (two groups, five steps, decay and
     no decay), sgd_ref against torch.optim.SGD(momentum=0.9, weight_decay), both to 1e-12 relative.  torch gets the float64 values
     of the fp32 constants; what the decimal literals would change in one update is printed.
  2. the host's fp32 sqrt, division, rsqrt and pow re-measured against float64 and compared with optim_ref.MATH_MEASURED
  3. the bounds hold for an fp32 emulation of the three forms of adam_elem (flat: the written-out fmas; chunk: m = fma(b1, m, ..),
     every other sum fused; matrix: m = fma(1 - b1, g, b1 m), everything else rounded on its own) and of sgd_elem, fma emulated
     through float64, over the operand sets, steps and variants below -- the case lists and check functions the GPU file imports.
     Every error / bound <= 1 with no element left out.
  4. exact tiers: three SGD steps on small integers with power-of-two rates, and AdamW with g = m = v = 0 (p' = p (1 - lr wd), dyadic)
     or lr = 0 (p' keeps the bits of p), have one legal value per element: the emulator reproduces it bit for bit in every form.

Worst error / bound of the emulator over all sets, steps and variants (each test prints its own).  One u per rounding is a sharp
count: m and v take two to four roundings and come close to it.
  flat     m 0.96  v 0.98  p 0.48  gnorm_out 0.29      p at step 2 / 7 alone: 0.47 / 0.48
  chunk    m 0.50  v 0.50  p 0.78                      p at step 2 / 7 alone: 0.75 / 0.78
  matrix   m 0.96  v 0.98  p 0.78                      p at step 2 / 7 alone: 0.75 / 0.78
  SGD      m 0.87  p 1.00 (the last fma rounds p' itself: half an ulp of a value just above a power of two is u |p'|)
Host fp32 against float64, in u: sqrt 1.05, division 1.00, rsqrt 1.50, pow 1.00; the device is allowed twice that.  The relative bound
of 1 / sqrt(bc2) is 1003 u at step 1, 503 u at step 2, 146 u at step 7 and 4.1 u at step 1000.
Median |update| / ulp(p) at step 7: randn 88, cancel 0.04 (m' nearly cancels), eps 240, wide 7400, sharp 2.3e6 -- with |p| ~ 1 an ulp
of p hides all but the coarsest error of the update; the sharp set is what sees the update's own arithmetic.  One update computed
with the decimal literals instead of the fp32 constants differs by 0.8 u.
"""
import pytest
import torch

from oracle import optim_ref as R
from test_region_fp64_gpu import Worst, hold

F = torch.float32
FORMS = ("flat", "chunk", "mat")
N_FLAT = 12296
# eight ranges whose boundaries are multiples of 4 and no multiples of 1024 (they fall inside a workgroup's stride), every (lr, wd)
# different, one without decay, and a gap of 8 elements (5004 .. 5011) that no range covers
RANGES8 = [(0, 1028, 1e-4, 1e-4), (1028, 2060, 5e-5, 1e-2), (2060, 4108, 2e-4, 1e-4), (4108, 5004, 1e-5, 1e-3), (5012, 6148, 3e-4, 0.0),
           (6148, 8196, 7e-5, 1e-1), (8196, 10244, 1e-3, 1e-4), (10244, N_FLAT, 2e-5, 5e-2)]
SPAN = (4100, 8200)
# name -> what differs from: fp32 gradients, the step by value, the rates by value, the clip engaged, grad_scale 1, the whole buffer
VARIANTS = {
    "plain": {},
    "step_dev, a contradicting step by value": dict(step_dev=True),
    "bf16 gradients": dict(g16=True),
    "lr_dev, contradicting rates by value": dict(lr_dev=True),
    "clip not engaged": dict(clip="idle"),
    "max_norm 0, no gnorm_sq": dict(clip="off"),
    "grad_scale 0.5": dict(grad_scale=0.5),
    "span (4100, 8200)": dict(span=SPAN),
}


# ------------------------------------------------------------------------------------------------ specs (shared with the GPU file)
def adam_spec(kind, n, seed, step, ranges, *, span=None, grad_scale=1.0, clip="engaged", g16=False, step_dev=False, lr_dev=False, own=None,
              beta1=0.9, beta2=0.999, eps=1e-8):
    """One AdamW launch: operands of set `kind`, the fp32 word of sum g^2 computed in float64 (the order of the norm's atomics stays
    out of the element bounds), max_norm half (engaged) or twice (idle) the total norm, or 0 with no word at all (off)."""
    g = torch.Generator().manual_seed(seed)
    clip_of = {}

    def gs_of(gr):
        sq = R.f32(R.sqnorm_ref(gr))
        total = sq ** 0.5 * R.f32(grad_scale)
        mx = {"engaged": R.f32(total / 2), "idle": R.f32(total * 2), "off": 0.0}[clip]
        clip_of.update(sq=sq if clip != "off" else None, max_norm=mx)
        clip_of["clip"] = R.clip_ref(clip_of["sq"], grad_scale, mx)
        return clip_of["clip"].gs
    p, gr, m, v = R.operands(kind, n, g, bf16_grads=g16, gs_of=gs_of, beta1=beta1)
    gs_of(gr)
    if own is None:
        own = torch.zeros(n, dtype=torch.bool)
        b, e = span if span is not None else (0, n)
        own[b:e] = True
    return dict(kind=kind, n=n, step=step, ranges=ranges, span=span, grad_scale=grad_scale, g16=g16, step_dev=step_dev, lr_dev=lr_dev, own=own,
                beta1=beta1, beta2=beta2, eps=eps, p=p, g=gr, m=m, v=v, **clip_of)


def flat_specs(kind, variant):
    """the flat pass of one operand set and variant at every step of optim_ref.STEPS"""
    return [adam_spec(kind, N_FLAT, 100 + i, step, RANGES8, **VARIANTS[variant]) for i, step in enumerate(R.STEPS)]


def dyadic_ranges(ranges, only=None):
    """the same element ranges with power-of-two lr (2^-3 .. 2^-6) and wd (2^-1, 2^-2, 0); only: every other range gets lr = wd = 0"""
    return [(b, e, 2.0 ** -(3 + i % 4) if only in (None, i) else 0.0, (0.5, 0.25, 0.0)[i % 3] if only in (None, i) else 0.0)
            for i, (b, e, _, _) in enumerate(ranges)]


def probe_spec(n, ranges, *, lr_zero=False, span=None, own=None):
    """the exact AdamW probes: g = m = v = 0, p = k / 64 with |k| <= 2000 and k != 0.  Dyadic lr, wd: p' = p (1 - lr wd) exactly.
    lr_zero: lr = 0 beside a decay that must not act, p' has the bits of p."""
    g = torch.Generator().manual_seed(77)
    k = torch.randint(1, 2001, (n,), generator=g).double() * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    z = torch.zeros(n, dtype=torch.float64)
    if lr_zero:
        ranges = [(b, e, 0.0, w) for b, e, _, w in ranges]
    spec = adam_spec("randn", n, 0, 3, ranges, span=span, clip="off", own=own)
    spec.update(p=k / 64, g=z, m=z.clone(), v=z.clone(), exact=True)
    return spec


def sgd_spec(kind, n, seed, ranges, *, span=None, clip="engaged", g16=False):
    spec = adam_spec("randn", n, seed, 1, ranges, span=span, clip=clip, g16=g16)
    if kind == "ints":                    # gs = 1, momentum 0.5, power-of-two rates, integers: at most 12 fraction bits after three steps
        g = torch.Generator().manual_seed(seed)
        ints = lambda: torch.randint(-8, 9, (n,), generator=g).double()          # noqa: E731
        spec.update(p=ints(), g=ints(), m=ints(), beta1=0.5, exact=True,
                    ranges=[(b, e, (0.5, 0.25)[i % 2], (0.5, 0.25, 0.0)[i % 3]) for i, (b, e, _, _) in enumerate(ranges)])
    return spec


# ------------------------------------------------------------------------------------------------ checks (shared with the GPU file)
def _unowned_kept(tag, spec, got, names):
    rest = ~spec["own"]
    for k in names:
        same = got[k][rest] == spec[k][rest]
        assert bool(same.all()), f"{tag} {k}: {int((~same).sum())} elements the call does not own were changed"


def _adam_ref(spec):
    c = spec["clip"]
    return R.adamw_ref(spec["p"], spec["g"], spec["m"], spec["v"], spec["ranges"], spec["step"], gs=c.gs, d_gs=c.d_gs, beta1=spec["beta1"],
                       beta2=spec["beta2"], eps=spec["eps"])


def hold_region(w, tag, spec, got, ref, mask):
    """m', v', p' of the elements in `mask` at the bounds (exact specs: a zero bound)"""
    z = 0.0 if spec.get("exact") else 1.0
    for k, r, b in (("m", ref.m, ref.bound_m), ("v", ref.v, ref.bound_v), ("p", ref.p, ref.bound_p)):
        hold(w, f"{tag}{k}", got[k][mask], r[mask], b[mask] * z)


def check_adamw(w, tag, spec, got, ref=None):
    """got: p, m, v (float64, the whole buffers) and gnorm_out after the launch.  Owned elements at the bounds, everything else
    unchanged; owned elements that no range covers (or whose lr is 0) keep the bits of p while m and v advance."""
    ref = _adam_ref(spec) if ref is None else ref
    own = spec["own"]
    _unowned_kept(tag, spec, got, ("p", "m", "v"))
    hold_region(w, tag, spec, got, ref, own)
    lr, wd = R.range_values(spec["n"], spec["ranges"])
    idle = own & (lr == 0)                # the update is 0 and 1 - 0 wd is 1 exactly
    assert bool((got["p"][idle] == spec["p"][idle]).all()), f"{tag}p: an element with lr = 0 moved"
    if got.get("gnorm_out") is not None:
        c = spec["clip"]
        hold(w, f"{tag}gnorm_out", torch.tensor([got["gnorm_out"]], dtype=torch.float64), torch.tensor([c.total], dtype=torch.float64), c.bound_total)
    return ref


def check_sgd(w, tag, spec, got, steps=1):
    """`steps` SGD steps of the same gradient (got: after the last one)"""
    c = spec["clip"]
    p, m = spec["p"], spec["m"]
    bp, bm = torch.zeros_like(p), torch.zeros_like(p)
    for _ in range(steps):
        ref = R.sgd_ref(p, spec["g"], m, spec["ranges"], gs=c.gs, d_gs=c.d_gs, momentum=spec["beta1"])
        p, m, bp, bm = ref.p, ref.m, bp + ref.bound_p, bm + ref.bound_m          # (more than one step: exact specs only)
    assert steps == 1 or spec.get("exact")
    own = spec["own"]
    _unowned_kept(tag, spec, got, ("p", "m"))
    z = 0.0 if spec.get("exact") else 1.0
    hold(w, f"{tag}m", got["m"][own], m[own], bm[own] * z)
    hold(w, f"{tag}p", got["p"][own], p[own], bp[own] * z)


def update_ulps(spec):
    """median |update| / ulp(p) over the owned elements with lr > 0"""
    ref = _adam_ref(spec)
    lr, _ = R.range_values(spec["n"], spec["ranges"])
    on = spec["own"] & (lr > 0) & (spec["p"] != 0)
    ulp = 2.0 ** (torch.floor(torch.log2(spec["p"][on].abs())) - 23)
    return float((ref.upd[on].abs() / ulp).median())


# ------------------------------------------------------------------------------------------------ the fp32 emulation
def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def t32(x):
    return torch.tensor(x, dtype=torch.float64).float()


class Emulator:
    """the arithmetic of adam_coef / clip_scale / adam_range / adam_elem / sgd_elem in fp32 on the CPU, one contraction choice per form"""

    def __init__(self, form):
        self.form = form

    @staticmethod
    def coef(spec, sgd=False):
        gsc, mx = t32(spec["grad_scale"]), t32(spec["max_norm"])
        total = (t32(spec["sq"]) if spec["sq"] is not None else t32(0.0)).sqrt() * gsc
        coef = torch.minimum(t32(1.0), mx / (total + t32(1e-6))) if float(mx) > 0 else t32(1.0)
        gs = gsc * coef
        if sgd:
            return gs, total, None, None
        st = t32(float(spec["step"]))
        bc1 = 1 - torch.pow(t32(spec["beta1"]), st)
        isb2 = torch.rsqrt(1 - torch.pow(t32(spec["beta2"]), st))
        return gs, total, bc1, isb2

    @staticmethod
    def state(spec):
        lr, wd = R.range_values(spec["n"], spec["ranges"])
        return [spec[k].float() for k in ("p", "g", "m", "v")] + [lr.float(), wd.float()]

    def adamw(self, spec):
        gs, total, bc1, isb2 = self.coef(spec)
        p, g, m, v, lr, wd = self.state(spec)
        b1, b2, eps = t32(spec["beta1"]), t32(spec["beta2"]), t32(spec["eps"])
        gg = g * gs
        if self.form == "flat":
            m1 = fma(1 - b1, gg, b1 * m)
            v1 = fma(gg, (1 - b2) * gg, b2 * v)
            den = fma(v1.sqrt(), isb2, eps)
            p1 = fma(fma(-lr, wd, t32(1.0)), p, -((lr / bc1) * (m1 / den)))
        elif self.form == "chunk":
            p0 = p * fma(-lr, wd, t32(1.0))
            m1 = fma(b1, m, (1 - b1) * gg)
            v1 = fma(b2, v, ((1 - b2) * gg) * gg)
            den = fma(v1.sqrt(), isb2, eps)
            p1 = fma(-(lr / bc1), m1 / den, p0)
        else:
            p0 = p * (1 - lr * wd)
            m1 = fma(1 - b1, gg, b1 * m)
            v1 = b2 * v + ((1 - b2) * gg) * gg
            den = v1.sqrt() * isb2 + eps
            p1 = p0 - (lr / bc1) * (m1 / den)
        own = spec["own"]
        out = {k: torch.where(own, new.double(), spec[k]) for k, new in (("p", p1), ("m", m1), ("v", v1))}
        out["gnorm_out"] = float(total)
        return out

    def sgd(self, spec, steps=1):
        gs, total, _, _ = self.coef(spec, sgd=True)
        p, g, m, _, lr, wd = self.state(spec)
        b1 = t32(spec["beta1"])
        for _ in range(steps):
            m = fma(b1, m, fma(g, gs, wd * p))
            p = fma(-lr, m, p)
        own = spec["own"]
        return dict(p=torch.where(own, p.double(), spec["p"]), m=torch.where(own, m.double(), spec["m"]), gnorm_out=float(total))


# ------------------------------------------------------------------------------------------------ 1. pinned to torch
def _groups(n):
    return [(0, n // 2, 1e-3, 1e-2), (n // 2, n, 1e-4, 0.0)]


def test_adamw_ref_and_clip_ref_equal_torch_adamw_behind_clip_grad_norm():
    n, steps = 512, 5
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    ranges = _groups(n)
    b1, b2, eps, mx = R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(0.1)
    a, b = torch.nn.Parameter(p0[:n // 2].clone()), torch.nn.Parameter(p0[n // 2:].clone())
    opt = torch.optim.AdamW([dict(params=[a], lr=R.f32(ranges[0][2]), weight_decay=R.f32(ranges[0][3])),
                             dict(params=[b], lr=R.f32(ranges[1][2]), weight_decay=R.f32(ranges[1][3]))], betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, steps + 1):
        gr = torch.randn(n, generator=gen, dtype=torch.float64)
        a.grad, b.grad = gr[:n // 2].clone(), gr[n // 2:].clone()
        total = torch.nn.utils.clip_grad_norm_([a, b], mx)
        opt.step()
        c = R.clip_ref(R.sqnorm_ref(gr), 1.0, mx, word=False)
        assert abs(c.total - float(total)) <= 1e-12 * float(total)
        gs = c.gs
        ref = R.adamw_ref(p, gr, m, v, ranges, step, gs=gs)
        p, m, v = ref.p, ref.m, ref.v
        want = torch.cat([a.detach(), b.detach()])
        assert float((p - want).abs().max()) <= 1e-12 * float(want.abs().max()), step
    st = opt.state[a]
    assert float((m[:n // 2] - st["exp_avg"]).abs().max()) <= 1e-12 * float(st["exp_avg"].abs().max())
    assert float((v[:n // 2] - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max())
    # clip_ref itself, on a squared norm that is an fp32 number: torch's coefficient to 1e-12 (torch clamps max_norm / (total + 1e-6) at 1)
    for sq, gsc, mxn in ((4.0, 1.0, 0.1), (4.0, 0.5, 0.1), (2.0 ** -14, 1.0, 0.1), (2.25, 1.0, 0.0)):
        c = R.clip_ref(sq, gsc, mxn)
        total = sq ** 0.5 * gsc
        want = gsc * min(1.0, R.f32(mxn) / (total + R.f32(1e-6))) if mxn > 0 else gsc
        assert abs(c.total - total) <= 1e-12 * total and abs(c.gs - want) <= 1e-12 * want
    # what the decimal literals would change in one update: beta2 = 0.999 against float32(0.999), step 1
    one = R.adamw_ref(p0, gr, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), ranges, 1)
    lit = (1e-3 * gr / ((gr * gr * (1 - 0.999)).sqrt() / (1 - 0.999) ** 0.5 + 1e-8) * (1 - 0.9) / (1 - 0.9))[:n // 2]
    rel = float(((one.upd[:n // 2] - lit).abs() / lit.abs()).max())
    print(f"\n[literals] one update with decimal literals instead of the fp32 constants: {rel:.2e} relative = {rel / R.U:.1f} u")


def test_sgd_ref_equals_torch_sgd_with_momentum_and_weight_decay():
    n, steps = 512, 5
    gen = torch.Generator().manual_seed(2)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    ranges = [(0, n // 2, 1e-2, 1e-2), (n // 2, n, 1e-3, 0.0)]
    mom, mx = R.f32(0.9), R.f32(0.1)
    a, b = torch.nn.Parameter(p0[:n // 2].clone()), torch.nn.Parameter(p0[n // 2:].clone())
    opt = torch.optim.SGD([dict(params=[a], lr=R.f32(1e-2), weight_decay=R.f32(1e-2)), dict(params=[b], lr=R.f32(1e-3), weight_decay=0.0)],
                          lr=1.0, momentum=mom)
    p, m = p0.clone(), torch.zeros(n, dtype=torch.float64)
    for step in range(1, steps + 1):
        gr = torch.randn(n, generator=gen, dtype=torch.float64)
        a.grad, b.grad = gr[:n // 2].clone(), gr[n // 2:].clone()
        torch.nn.utils.clip_grad_norm_([a, b], mx)
        opt.step()
        gs = min(1.0, mx / (R.sqnorm_ref(gr) ** 0.5 + R.f32(1e-6)))
        ref = R.sgd_ref(p, gr, m, ranges, gs=gs, momentum=mom)
        p, m = ref.p, ref.m
        want = torch.cat([a.detach(), b.detach()])
        assert float((p - want).abs().max()) <= 1e-12 * float(want.abs().max()), step
    buf = torch.cat([opt.state[a]["momentum_buffer"], opt.state[b]["momentum_buffer"]])
    assert float((m - buf).abs().max()) <= 1e-12 * float(buf.abs().max())


# ------------------------------------------------------------------------------------------------ 2. the math functions
def test_host_math_errors_are_what_optim_ref_records():
    got = R.measure_math_err()
    print("\n[math] host fp32 against float64, in u = 2^-24: " + "  ".join(f"{k}={v:.2f}" for k, v in got.items())
          + "   allowed on the device: " + "  ".join(f"{k}={v:.2f}" for k, v in R.MATH_ERR.items()))
    for k, v in got.items():
        assert v <= R.MATH_MEASURED[k] * 1.01 + 0.01, (k, v)
        assert v >= R.MATH_MEASURED[k] * 0.8, (k, v, "the recorded constant is stale")
    c = R.bias_corrections(1, 0.9, 0.999)
    print(f"[math] relative bound of 1/sqrt(bc2) in u: step 1 {c.d_isb2 / R.U:.0f}, step 2 {R.bias_corrections(2, 0.9, 0.999).d_isb2 / R.U:.0f}, "
          f"step 7 {R.bias_corrections(7, 0.9, 0.999).d_isb2 / R.U:.0f}, step 1000 {R.bias_corrections(1000, 0.9, 0.999).d_isb2 / R.U:.1f}")
    assert float(torch.pow(t32(0.999), t32(float(R.STEPS[-1])))) == 0.0        # the last step of the list underflows


def test_norm_chain_and_bound():
    assert R.sqnorm_chain(1, False) == 1 + 3 + 0 + 1 + 6 + 4 + 1
    assert R.sqnorm_chain(3 * 2 ** 20 + 5, False) == 1 + 3 + 2 + 1 + 6 + 4 + 2048
    assert R.sqnorm_chain(5 * 2 ** 20 + 11, True) == 1 + 2 * 8 + 1 + 6 + 4 + 2048
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(1027, generator=g) + 3).double()
    seq = torch.zeros((), dtype=F)
    for e in x.float():                              # the longest chain there is: one element after the other
        seq = seq + e * e
    assert abs(float(seq) - R.sqnorm_ref(x)) <= ((1 + R.U) ** 1028 - 1) * R.sqnorm_ref(x)


# ------------------------------------------------------------------------------------------------ 3. the bounds on the emulation
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", R.OPERAND_SETS)
def test_emulated_adamw_forms_stay_inside_the_bounds(kind, variant):
    w = Worst()
    for spec in flat_specs(kind, variant):
        for form in FORMS:
            ws = Worst()
            check_adamw(ws, f"{form} ", spec, Emulator(form).adamw(spec))
            for k, v in ws.items():
                w.note(k, v)
            if spec["step"] in (2, 7):
                w.note(f"{form} p at step {spec['step']}", ws[f"{form} p"])
    print(w.line(f"emulated {kind}, {variant}"))
    if variant == "plain":
        print(f"[{kind}] median |update| / ulp(p) at step 7: {update_ulps(flat_specs(kind, variant)[2]):.3g}")


@pytest.mark.parametrize("kind", ["randn", "ints"])
def test_emulated_sgd_stays_inside_the_bound_and_the_integer_tier_is_exact(kind):
    w = Worst()
    for variant in ("plain", "span (4100, 8200)", "bf16 gradients"):
        kw = {k: v for k, v in VARIANTS[variant].items() if k in ("span", "g16")}
        spec = sgd_spec(kind, N_FLAT, 31, RANGES8, clip="off" if kind == "ints" else "engaged", **kw)
        steps = 3 if kind == "ints" else 1
        check_sgd(w, "sgd ", spec, Emulator("flat").sgd(spec, steps), steps)
    print(w.line(f"emulated sgd {kind}"))


def test_emulated_exact_adamw_probes_have_one_value_in_every_form():
    w = Worst()
    for form in FORMS:
        for span in (None, SPAN):
            for tag, lr_zero in (("decay", False), ("lr 0", True)):
                spec = probe_spec(N_FLAT, dyadic_ranges(RANGES8), lr_zero=lr_zero, span=span)
                check_adamw(w, f"{form} {tag} ", spec, Emulator(form).adamw(spec))
        for r in range(len(RANGES8)):
            spec = probe_spec(N_FLAT, dyadic_ranges(RANGES8, only=r))
            check_adamw(w, f"{form} range {r} ", spec, Emulator(form).adamw(spec))
    assert all(v == 0.0 for v in w.values())
