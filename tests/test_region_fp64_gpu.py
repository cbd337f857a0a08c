"""GPU: the few-row region (rt_qenc_fwd, rt_qenc_bwd, rt_head_loss, the decoder launches and the launched chains they replace)
stage by stage against float64 (oracle/region_ref.py, pinned to the oracle by tests/test_region_ref_cpu.py).

Teacher forcing: these kernels store every intermediate, so each stage is recomputed in float64 FROM THE TENSORS THE KERNEL ITSELF
READ FOR IT and compared element by element, no exclusions.  No ReLU gate can flip and no bf16 noise runs free, so the bounds
follow from the number formats instead of from measurements (u = 2^-23):

  fp32 product of K terms     |got - ref| <= (K + 2) u (|x| |w|^T + |b|)          (also covers a truncating adder)
  bf16 result                 the stage's bound + 2^-8 |ref|                      (half an ulp + a double-rounding flip; ReLU is
                                                                                   1-Lipschitz: no special case around zero)
  LayerNorm / softmax stages  (__expf, rsqrt) the per-kernel gates of tests/test_ops_gpu.py, PER ROW: rel-L2 1e-5 forward,
                              2e-5 backward, 1e-4 for the query attention's backward; bf16 results add 2^-8 |ref| per element
  row statistics              mean = sum x / D is a product of K = D terms; rstd: the variance is a sum of D squares of rounded
                              differences ((D + 4) u relative), halved by the rsqrt, + 2 ulp of rsqrtf: (D / 2 + 6) u rstd
  softmax weights             take the SCORES' product bound through the softmax first (the scores are not stored):
                              d qw_l <= qw_l (d s_l + sum_j qw_j d s_j); the row gate holds what exceeds that.  The same for the
                              attention backward's d s = qw (dw - sum qw dw), whose difference cancels: dw's product bound is
                              carried through d s into d q / d k before the 1e-4 row gate
  sums of R rows              d gamma / d beta partials, bias gradients, d query_embed: (R + c) u sum |terms|, c = the extra
                              additions of the kernel's reduction tree (stated at each use)
  copies / masked elements    exact: cls16, lang16, dropped elements, invalid phrases, memory rows the launch does not own

The backward stages take their gates from the kernel's own stored activations (y1 > 0, y2 > 0, hdn != 0) or, where the kernel
re-evaluates the LayerNorm's sign (rt_ln_bwd_group, contraction off), from the same fp32 operations in the same order on the host.

Decoder runs with dropout on stay with the bit-identity tests of tests/test_decoder_coop_gpu.py; the decoder stages here run
in eval mode.

Worst error / bound per stage over all cases, measured on the MI355X (every run prints them per case).  bf16 stores sit just under 1
because half an ulp is the rounding everyone of them makes; fp32 products and the row-gated stages use a few per cent of their bound:
  rt_head_loss:
    hmean 0.00, hrstd 0.01, hs16 0.00, y1 0.95, y2 0.96, logits 0.00, losses 0.03, dlogits 0.00, dl16 0.91, total 0.11
    dy2 0.99, dy1 0.95, dhs 0.00, dnorm 0.00, part_n 0.05, db2_part 0.01, G bbox weight 0.10, G bbox bias 0.00, G norm 0.12
    G b2 0.12
  launched head:
    hmean 0.00, hrstd 0.01, hs16 0.00, y1 0.95, y2 0.96, logits 0.00, losses 0.03, dlogits 0.00, total 0.08, dy2 0.99
    dy1 0.95, dhs 0.00, dnorm 0.00, G bbox weight 0.10, G bbox bias 0.00, G norm 0.08
  qenc fwd fused:
    cls16 0.00, lang16 0.00, kq 0.00, qs 0.00, vs 0.00, qw 0.00, c16 0.99, co 0.00, ln mean 0.00, ln rstd 0.01
    cat16[:, :E] 0.00, t1 0.00, a16 0.00, t2 0.00, tgt32 0.01, qpos 0.01, tgt16 0.99, tgtq16 1.00
  qenc fwd chain:
    cls16 0.00, lang16 0.00, kq 0.00, qs 0.00, vs 0.00, qw 0.00, c16 0.99, co 0.00, ln mean 0.00, ln rstd 0.01
    cat16[:, :E] 0.00, t1 0.00, a16 0.00, t2 0.00, tgt32 0.01, qpos 0.01, tgt16 0.99, tgtq16 1.00
  qenc bwd fused:
    dt2b 0.00, da 0.00, dt1b 0.00, dcat 0.00, dcob 0.00, dc 0.00, dk16 0.00, dqs16 0.00, dvs16 0.00, part5 0.06, part1 0.07
    partc 0.05, dqembed 0.09, dmem lang 0.00, dmem cls 0.00, G weight 0.19, G bias 0.09, G ln 0.15
  qenc bwd chain:
    dt2b 0.00, da 0.00, dt1b 0.00, dcat 0.00, dcob 0.00, dc 0.00, dk16 0.00, dqs16 0.00, dvs16 0.00, G ln 0.05, dqembed 0.07
    dmem lang 0.00, dmem cls 0.00, G weight 0.15, G bias 0.12        (with the two-query shape: d query_embed [2, 2E] 0.06)
  decoder fwd:
    sa o 0.94, u 0.00, ln mean 0.00, ln rstd 0.01, t1q16 0.00, q2 0.93, k2 0.97, v2 0.95, o2 0.02, lse2 0.01, u2 0.00
    t2_16 0.00, hdn 0.95, u3 0.00, t3 0.01, t3_16 0.99, sa v 0.94, sa qk 0.94, sa lse 0.01, t3q16 0.95

(d) floor / measured / gate per tensor (rel-L2 per tensor against the exact twin; L<i> = vl_transformer.decoder.layers.<i>; the
cooperative cases with the packed memory-gradient product -- the per-layer form differs only in `mem` / `memp`, listed below):
  tensor                             |         single-B2          |         single-B13         |          multi-B2         
  tgt                                | 3.84e-03 3.84e-03 1.15e-02 | 3.12e-03 3.14e-03 9.37e-03 | 3.94e-03 4.45e-03 1.18e-02
  qpos                               | 1.78e-02 1.78e-02 3.00e-02 | 1.10e-02 1.10e-02 3.00e-02 | 1.64e-02 1.94e-02 3.00e-02
  mem                                | 3.31e-03 3.31e-03 9.92e-03 | 3.41e-03 3.40e-03 1.02e-02 | 3.57e-03 3.92e-03 1.07e-02
  memp                               | 6.98e-03 6.98e-03 2.09e-02 | 5.58e-03 5.56e-03 1.67e-02 | 5.50e-03 6.21e-03 1.65e-02
  L1.self_attn.in_proj_weight        | 3.30e-03 3.30e-03 9.90e-03 | 3.06e-03 3.07e-03 9.19e-03 | 5.52e-03 5.04e-03 1.66e-02
  L1.self_attn.in_proj_bias          | 3.30e-03 3.30e-03 9.91e-03 | 3.05e-03 3.05e-03 9.14e-03 | 4.56e-03 4.35e-03 1.37e-02
  L1.self_attn.out_proj.weight       | 2.91e-03 2.91e-03 8.74e-03 | 2.46e-03 2.46e-03 7.38e-03 | 2.44e-03 2.50e-03 7.33e-03
  L1.self_attn.out_proj.bias         | 2.91e-03 2.91e-03 8.75e-03 | 2.45e-03 2.45e-03 7.34e-03 | 2.44e-03 2.50e-03 7.33e-03
  L1.multihead_attn.in_proj_weight   | 4.52e-03 4.52e-03 1.36e-02 | 3.49e-03 3.47e-03 1.05e-02 | 3.37e-03 3.39e-03 1.01e-02
  L1.multihead_attn.in_proj_bias     | 4.10e-03 4.10e-03 1.23e-02 | 3.27e-03 3.25e-03 9.80e-03 | 3.14e-03 3.16e-03 9.41e-03
  L1.multihead_attn.out_proj.weight  | 2.29e-03 2.29e-03 6.88e-03 | 2.11e-03 2.11e-03 6.35e-03 | 2.06e-03 2.06e-03 6.19e-03
  L1.multihead_attn.out_proj.bias    | 2.30e-03 2.30e-03 6.89e-03 | 2.11e-03 2.10e-03 6.32e-03 | 2.06e-03 2.05e-03 6.17e-03
  L1.linear1.weight                  | 2.48e-03 2.48e-03 7.44e-03 | 2.27e-03 2.27e-03 6.80e-03 | 2.29e-03 2.29e-03 6.87e-03
  L1.linear1.bias                    | 2.48e-03 2.48e-03 7.45e-03 | 2.26e-03 2.26e-03 6.79e-03 | 2.29e-03 2.29e-03 6.86e-03
  L1.linear2.weight                  | 1.73e-03 1.73e-03 5.20e-03 | 1.59e-03 1.59e-03 4.77e-03 | 1.64e-03 1.64e-03 4.91e-03
  L1.linear2.bias                    | 1.73e-03 1.73e-03 5.20e-03 | 1.59e-03 1.59e-03 4.76e-03 | 1.63e-03 1.64e-03 4.91e-03
  L1.norm1.weight                    | 2.74e-03 2.74e-03 8.24e-03 | 1.85e-03 1.84e-03 5.55e-03 | 1.85e-03 1.66e-03 5.55e-03
  L1.norm1.bias                      | 2.41e-03 2.41e-03 7.22e-03 | 1.83e-03 1.83e-03 5.50e-03 | 1.74e-03 1.63e-03 5.23e-03
  L1.norm2.weight                    | 1.62e-03 1.62e-03 4.85e-03 | 1.27e-03 1.27e-03 3.80e-03 | 1.19e-03 1.18e-03 3.56e-03
  L1.norm2.bias                      | 1.57e-03 1.57e-03 4.71e-03 | 1.29e-03 1.29e-03 3.88e-03 | 1.36e-03 1.36e-03 4.09e-03
  L1.norm3.weight                    | 0.00e+00 5.71e-08 1.00e-06 | 0.00e+00 6.78e-08 1.00e-06 | 0.00e+00 7.56e-08 1.00e-06
  L1.norm3.bias                      | 0.00e+00 2.56e-08 1.00e-06 | 0.00e+00 5.40e-08 1.00e-06 | 0.00e+00 4.38e-08 1.00e-06
  L0.self_attn.in_proj_weight        | 4.19e-03 4.19e-03 1.26e-02 | 3.10e-03 3.19e-03 9.31e-03 | 4.26e-03 7.30e-03 1.28e-02
  L0.self_attn.in_proj_bias          | 4.19e-03 4.19e-03 1.26e-02 | 3.07e-03 3.16e-03 9.21e-03 | 3.55e-03 4.81e-03 1.07e-02
  L0.self_attn.out_proj.weight       | 3.98e-03 3.98e-03 1.19e-02 | 2.60e-03 2.65e-03 7.81e-03 | 3.24e-03 3.33e-03 9.72e-03
  L0.self_attn.out_proj.bias         | 3.99e-03 3.99e-03 1.20e-02 | 2.56e-03 2.61e-03 7.69e-03 | 3.24e-03 3.33e-03 9.71e-03
  L0.multihead_attn.in_proj_weight   | 6.21e-03 6.21e-03 1.86e-02 | 4.51e-03 4.39e-03 1.35e-02 | 5.00e-03 5.37e-03 1.50e-02
  L0.multihead_attn.in_proj_bias     | 5.39e-03 5.39e-03 1.62e-02 | 3.95e-03 3.82e-03 1.18e-02 | 4.25e-03 4.67e-03 1.27e-02
  L0.multihead_attn.out_proj.weight  | 2.77e-03 2.77e-03 8.32e-03 | 2.23e-03 2.16e-03 6.70e-03 | 2.54e-03 2.60e-03 7.63e-03
  L0.multihead_attn.out_proj.bias    | 2.77e-03 2.77e-03 8.32e-03 | 2.21e-03 2.13e-03 6.63e-03 | 2.53e-03 2.60e-03 7.60e-03
  L0.linear1.weight                  | 3.10e-03 3.10e-03 9.30e-03 | 2.85e-03 2.86e-03 8.56e-03 | 2.96e-03 2.84e-03 8.87e-03
  L0.linear1.bias                    | 3.10e-03 3.10e-03 9.31e-03 | 2.85e-03 2.86e-03 8.57e-03 | 2.95e-03 2.83e-03 8.86e-03
  L0.linear2.weight                  | 2.55e-03 2.55e-03 7.66e-03 | 2.33e-03 2.33e-03 6.98e-03 | 2.49e-03 2.26e-03 7.46e-03
  L0.linear2.bias                    | 2.56e-03 2.56e-03 7.67e-03 | 2.33e-03 2.33e-03 6.98e-03 | 2.48e-03 2.26e-03 7.45e-03
  L0.norm1.weight                    | 4.87e-03 4.87e-03 1.46e-02 | 2.37e-03 2.29e-03 7.12e-03 | 2.95e-03 3.43e-03 8.86e-03
  L0.norm1.bias                      | 3.79e-03 3.79e-03 1.14e-02 | 2.20e-03 2.23e-03 6.61e-03 | 2.82e-03 2.90e-03 8.45e-03
  L0.norm2.weight                    | 2.56e-03 2.56e-03 7.67e-03 | 1.87e-03 1.84e-03 5.61e-03 | 2.20e-03 2.25e-03 6.59e-03
  L0.norm2.bias                      | 2.39e-03 2.39e-03 7.16e-03 | 1.74e-03 1.72e-03 5.21e-03 | 2.17e-03 2.15e-03 6.52e-03
  L0.norm3.weight                    | 1.74e-03 1.74e-03 5.22e-03 | 1.33e-03 1.37e-03 4.00e-03 | 2.11e-03 1.94e-03 6.33e-03
  L0.norm3.bias                      | 1.64e-03 1.64e-03 4.93e-03 | 1.38e-03 1.39e-03 4.14e-03 | 1.99e-03 1.80e-03 5.97e-03
  single-B2, per-layer memory gradient: mem 3.31e-03 3.31e-03 9.92e-03
  single-B2, per-layer memory gradient: memp 6.98e-03 6.98e-03 2.09e-02
  single-B13, per-layer memory gradient: mem 3.41e-03 3.40e-03 1.02e-02
  single-B13, per-layer memory gradient: memp 5.58e-03 5.56e-03 1.67e-02

In single-B2 the measured distance equals the floor to three digits: the kernels round where the twin rounds.  d query_pos's floor comes
from a rounding point that is no gradient rounding (the attention backward's delta from the stored bf16 output, see
_AttnDeltaFromStoredO); its gate is the 3e-2 cap.  The whole file (30 tests) takes 7 s on the MI355X.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import region_ref as R
from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state

pytestmark = pytest.mark.gpu

U32, U16 = 2.0 ** -23, 2.0 ** -8
FTZ = 2048 * 2.0 ** -126      # underflow: an operation may flush a subnormal to zero (2^-126 each); no element here takes 2048 operations
VT, QE = "vl_transformer.", "query_encoder."
REGION = (QE, VT + "decoder.", "bbox_embed.")
E = 256


# ------------------------------------------------------------------------------------------------ bounds and checks
def c64(t):
    return t.detach().to("cpu").double()


def pbound(x, W, b=None):
    """(K + 2) u (|x| |W|^T + |b|) for y = x W^T + b with K = x.shape[-1]"""
    m = x.abs() @ W.abs().transpose(-1, -2)
    return (x.shape[-1] + 2) * U32 * (m if b is None else m + b.abs())


def stat_bounds(x):
    D = x.shape[-1]
    _, rstd = R.ln_stats(x)
    return (D + 2) * U32 * x.abs().mean(-1), (D / 2 + 6) * U32 * rstd


class Worst(dict):
    """worst error / bound per stage of one test"""

    def note(self, name, ratio):
        self[name] = max(self.get(name, 0.0), float(ratio))

    def line(self, tag):
        return f"\n[{tag}] " + "  ".join(f"{k}={v:.2f}" for k, v in self.items())


def hold(w, name, got, ref, bound):
    """every element: |got - ref| <= bound (a zero bound: exact)"""
    got = c64(got).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    bound = torch.where(bound > 0, bound + FTZ, bound)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    w.note(name, worst)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        idx = np.unravel_index(i, tuple(ref.shape))
        raise AssertionError(f"{name}: element {idx}: got {float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} "
                             f"bound {float(bound.reshape(-1)[i]):.3e} (error / bound {worst:.2f})")


def hold_rows(w, name, got, ref, gate, slack=None, scale=None):
    """every row (last axis): || max(|got - ref| - slack, 0) || <= gate || scale row ||  (scale: ref itself unless given)"""
    got = c64(got).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs() - torch.where(ref != 0, FTZ, 0.0)
    err = (err if slack is None else err - slack).clamp(min=0)
    D = ref.shape[-1]
    en = err.reshape(-1, D).norm(dim=1)
    rn = gate * (ref if scale is None else scale).reshape(-1, D).norm(dim=1)
    ratio = torch.where(rn > 0, en / rn.clamp(min=1e-300), torch.where(en > 0, torch.full_like(en, float("inf")), torch.zeros_like(en)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    w.note(name, worst)
    i = int(ratio.argmax()) if ratio.numel() else 0
    assert worst <= 1.0, f"{name}: row {i}: excess {float(en[i]):.3e} over gate {float(rn[i]):.3e} (ratio {worst:.2f})"


def ln_sign_f32(x, mean, rstd, gam, bet):
    """rt_ln_bwd_group's ReLU gate: (x - mean) * rstd * gamma + beta > 0, each operation rounded to fp32 (contraction off)"""
    x, mean, rstd, gam, bet = (t.detach().float().cpu() for t in (x, mean, rstd, gam, bet))
    xh = (x - mean[:, None]) * rstd[:, None]
    return (xh * gam + bet) > 0


def rowsum_bound(terms, extra, mag=None):
    """sum over the rows (axis 0) of `terms`, accumulated in fp32 with up to rows + extra additions; mag: the terms' magnitudes where
    a term is itself a sum that can cancel (|a| + |b| instead of |a + b|)"""
    return (terms.shape[0] + extra) * U32 * (terms.abs() if mag is None else mag).sum(0)


# ------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def _model(nq):
    """One small model per n_q, shared by every test of this file.  The models carry state from test to test (train / eval, the
    gradient buffer flat_g, query_embed's gradient, _saved): a test sets what it reads before it launches (model.train / eval,
    flat_g.zero_(), its own start value of d query_embed) and leaves the model in eval mode; nothing a test reads is left over from
    the test before it.  _decoder_run below keeps each case's `_saved` record, which (c) and (d) share and only read."""
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.models.reftr_transformer import RefTR
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), n_q=nq)
    cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), n_q=nq)
    model = RefTR(cfg, device="cuda")
    model.load_state_dict(formula_state(param_shapes(ocfg)), strict=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    w2 = model.store.P["bbox_embed.layers.2.weight"]
    w2.copy_(0.02 * torch.randn(w2.shape, device="cuda", generator=g))          # a zero head hides everything behind it
    if nq > 1:
        qe = model.store.P[QE + "query_embed.weight"]
        qe.copy_(torch.randn(qe.shape, device="cuda", generator=g))
    model.mark_dirty(full=True)
    model.eval()
    model.refresh_now()
    crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
    return model, crit, ocfg


def params64(model):
    """The region's parameters as the kernels read them: weights = the bf16 operands (net.lins[...].W), biases and LayerNorm
    parameters = the fp32 masters."""
    st, net = model.store, model.net
    P = {k: c64(st.P[k]) for k in st.P if k.startswith(REGION)}
    for key, l in net.lins.items():
        if not key.startswith(REGION):
            continue
        assert torch.equal(l.WT, l.W.t()), key                  # the backward-data operand is the same values, transposed
        if key.endswith("."):
            P[key + "weight"] = c64(l.W)
    for i in range(model.cfg.dec_layers):
        p = f"{VT}decoder.layers.{i}."
        P[p + "self_attn.in_proj_weight"] = torch.cat([c64(net.lins[p + "self_attn.qk"].W), c64(net.lins[p + "self_attn.v"].W)])
        P[p + "multihead_attn.in_proj_weight"] = torch.cat([c64(net.lins[p + "multihead_attn." + k].W) for k in "qkv"])
    return P


# ================================================================================================ (a) rt_head_loss
HEAD_CASES = {
    "2x1": (2, 1, [[1], [1]]),
    "3x4": (3, 4, [[1, 1, 0, 0], [1, 0, 1, 1], [0, 0, 0, 0]]),          # ragged validity, one image without a valid phrase
    "8x1": (8, 1, [[1]] * 8),
    "2x16": (2, 16, [[1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0], [1] * 16]),      # the row limit per image
}


def _check_head(w, h, t3, P, w2, valid, targets, nb, weights, NL, fused):
    norm, mlp = VT + "decoder.norm.", "bbox_embed.layers."
    R_, N = t3.shape[0], t3.shape[0] // NL
    x = c64(t3)
    k = {n: c64(v) for n, v in h.items() if torch.is_tensor(v)}
    mean, rstd = R.ln_stats(x)
    bm, br = stat_bounds(x)
    hold(w, "hmean", h["hmean"], mean, bm)
    hold(w, "hrstd", h["hrstd"], rstd, br)
    f = R.head_forward(P, x, snap=lambda n, v: k[n])
    hold_rows(w, "hs16", h["hs16"], f["hs"], 1e-5, slack=U16 * f["hs"].abs())
    hold(w, "y1", h["y1"], f["y1"], pbound(k["hs16"], P[mlp + "0.weight"], P[mlp + "0.bias"]) + U16 * f["y1"].abs())
    hold(w, "y2", h["y2"], f["y2"], pbound(k["y1"], P[mlp + "1.weight"], P[mlp + "1.bias"]) + U16 * f["y2"].abs())
    hold(w, "logits", h["logits"], f["logits"], pbound(k["y2"], P[mlp + "2.weight"], P[mlp + "2.bias"]))
    # losses and d total / d logits at the kernel's own logits: rt_box_loss's gates (test_box_loss_against_golden_and_autograd:
    # 2e-6 absolute on a loss term, 1e-4 on d logits), the latter per row; invalid phrases exactly zero
    B, T = valid.shape
    losses, total, dl = R.head_losses(k["logits"].view(NL, B, T, 1, 4), valid, targets, nb, weights)
    hold(w, "losses", h["losses"], losses, 2e-6)
    dl = dl.reshape(R_, 4)
    hold_rows(w, "dlogits", h["dlogits"], dl, 1e-4)
    inval = (~valid).view(1, B * T).expand(NL, -1).reshape(-1)
    assert float(k["dlogits"].reshape(R_, 4)[inval].abs().sum()) == 0.0
    kdl = k["dlogits"].reshape(R_, 4)
    if fused:               # the launched head hands fp32 d logits to rt_small_dgrad: no bf16 copy
        hold(w, "dl16", h["dl16"], kdl, U16 * kdl.abs())
    terms = weights * k["losses"]       # sum of 2 NL weighted terms in fp32
    hold(w, "total", h["total"], terms.sum().reshape(1), (2 * NL + 2) * U32 * terms.abs().sum())
    b = R.head_backward(P, dict(t3=x, hstats=(k["hmean"], k["hrstd"]), y1=k["y1"], y2=k["y2"]), kdl, w2, snap=lambda n, v: k[n])
    g2, g1 = (k["y2"] > 0).double(), (k["y1"] > 0).double()
    hold(w, "dy2", h["dy2"], b["dy2"], g2 * ((4 + 2) * U32 * (kdl.abs() @ w2.abs()) + U16 * b["dy2"].abs()))
    hold(w, "dy1", h["dy1"], b["dy1"], g1 * (pbound(k["dy2"], P[mlp + "1.weight"].t()) + U16 * b["dy1"].abs()))
    hold(w, "dhs", h["dhs"], b["dhs"], pbound(k["dy1"], P[mlp + "0.weight"].t()))
    hold_rows(w, "dnorm", h["dnorm"], b["dnorm"], 2e-5)
    if fused:
        # per layer: the waves' row sums (<= ceil(N / 16) rows each), then 16 wave partials: <= N + 16 additions; x-hat and the
        # product add 4 roundings
        gr, br_ = b["dgamma_rows"].view(NL, N, E), b["dbeta_rows"].view(NL, N, E)
        for l in range(NL):
            hold(w, "part_n", h["part_n"][l, 0], gr[l].sum(0), rowsum_bound(gr[l], 16 + 4))
            hold(w, "part_n", h["part_n"][l, 1], br_[l].sum(0), rowsum_bound(br_[l], 16))
            # lane partials, a 6-level wave tree, 16 wave partials
            hold(w, "db2_part", h["db2_part"][l, 0], kdl.view(NL, N, 4)[l].sum(0), rowsum_bound(kdl.view(NL, N, 4)[l], 16 + 6))
        assert float(k["db2_part"][:, 1].abs().sum()) == 0.0
    return k


def _check_head_wgrads(w, st, k, NL, fused):
    """bbox_embed.layers.{0,1} and decoder.norm gradients from the kernel's own bf16 dy tensors, at the product bound"""
    mlp, norm = "bbox_embed.layers.", VT + "decoder.norm."
    for i, dy, x in ((1, k["dy2"], k["y1"]), (0, k["dy1"], k["hs16"])):
        rows = dy.shape[0]
        hold(w, "G bbox weight", st.G[f"{mlp}{i}.weight"], dy.t() @ x, (rows + 2) * U32 * (dy.abs().t() @ x.abs()))
        hold(w, "G bbox bias", st.G[f"{mlp}{i}.bias"], dy.sum(0), rowsum_bound(dy, 2))
    if fused:
        pn = k["part_n"]
        hold(w, "G norm", st.G[norm + "weight"], pn[:, 0].sum(0), rowsum_bound(pn[:, 0], 2))
        hold(w, "G norm", st.G[norm + "bias"], pn[:, 1].sum(0), rowsum_bound(pn[:, 1], 2))
        hold(w, "G b2", st.G[mlp + "2.bias"], k["db2_part"][:, 0].sum(0), rowsum_bound(k["db2_part"][:, 0], 2))


@pytest.mark.parametrize("case", list(HEAD_CASES))
def test_head_loss_stages_against_float64(hip, case):
    """rt_head_loss (all fifteen outputs + total), then the launched head on the same inputs (rt_layernorm_*, rt_conv_gemm,
    rt_box_loss, rt_small_dgrad) through the same checks, then the weight gradients both leave behind."""
    from reftr_amd.models.criterion import _box_weights
    from reftr_amd.models.net import RELU
    model, crit, ocfg = _model(1)
    model.eval()
    net, st = model.net, model.store
    B, Pn, v = HEAD_CASES[case]
    nq, NL = 1, model.cfg.dec_layers
    N = B * Pn
    g = torch.Generator(device="cuda").manual_seed(11 + N)
    t3 = torch.randn(NL * N, E, device="cuda", generator=g)
    valid = torch.tensor(v, dtype=torch.bool, device="cuda")
    nt = [int(n) for n in valid.sum(1).tolist()]
    tg = [{"boxes": torch.rand(n, 4, device="cuda", generator=g) * 0.4 + 0.3, "labels": torch.zeros(n, dtype=torch.long, device="cuda")} for n in nt]
    prepared = crit.prepare(tg, torch.device("cuda"))
    P = params64(model)
    w2 = c64(net.lins["bbox_embed.layers.2."].w32)
    weights = c64(_box_weights(crit, NL, t3.device))
    targets = [{"boxes": c64(t["boxes"])} for t in tg]
    nb = max(float(sum(nt)), 1.0)
    assert abs(float(prepared[2]) - nb) == 0.0
    vt = VT
    # ---- one launch
    w = Worst()
    st.flat_g.zero_()
    hs16 = torch.empty(NL * N, E, dtype=torch.bfloat16, device="cuda")
    h = model._head_loss_fused((crit, prepared), t3, hs16, valid, NL, B, Pn, nq, N)
    net._wgrad_only("bbox_embed.layers.1.", h["dy2"], h["y1"])
    net._wgrad_only("bbox_embed.layers.0.", h["dy1"], hs16)
    net.ln_batch.jobs.append(hip._desc(hip.LnPgJob, partials=h["part_n"], dgamma=st.G[vt + "decoder.norm.weight"],
                                       dbeta=st.G[vt + "decoder.norm.bias"], n_blocks=NL, D=E))
    net.ln_batch.jobs.append(hip._desc(hip.LnPgJob, partials=h["db2_part"], dgamma=net.lins["bbox_embed.layers.2."].gb, n_blocks=NL, D=4))
    net.flush_wgrads()
    torch.cuda.synchronize()
    k = _check_head(w, h, t3, P, w2, valid.cpu(), targets, nb, weights, NL, fused=True)
    _check_head_wgrads(w, st, k, NL, fused=True)
    print(w.line(f"rt_head_loss B={B} P={Pn}"))
    # ---- the launched head
    w = Worst()
    st.flat_g.zero_()
    hs16 = torch.empty(NL * N, E, dtype=torch.bfloat16, device="cuda")
    _, _, _, hm, hr = net.ln_fwd(t3, vt + "decoder.norm.", y_bf16=hs16, want_f32=False)
    y1, _ = net.lin_fwd("bbox_embed.layers.0.", hs16, act=RELU)
    y2, _ = net.lin_fwd("bbox_embed.layers.1.", y1, act=RELU)
    _, logits = net.lin_fwd("bbox_embed.layers.2.", y2, out_bf16=False, out_f32=True)
    losses, total, dl = hip.box_loss(logits.view(NL, B, Pn, nq, 4), valid.to(torch.uint8).contiguous(), *prepared, want_grad=True,
                                     weights=_box_weights(crit, NL, logits.device))
    dl = dl.reshape(NL * N, 4)
    l2 = net.lins["bbox_embed.layers.2."]
    dy2 = hip.small_dgrad(dl, l2.w32, gate=y2)
    dy1, _ = net.lin_bwd("bbox_embed.layers.1.", dy2, y1, gate=y1)
    _, dhs = net.lin_bwd("bbox_embed.layers.0.", dy1, hs16, out_bf16=False, out_f32=True)
    dnorm, _ = net.ln_bwd(dhs, t3, vt + "decoder.norm.", hm, hr, want_bf16=False)
    net.flush_wgrads()
    torch.cuda.synchronize()
    hl = dict(hs16=hs16, hmean=hm, hrstd=hr, y1=y1, y2=y2, logits=logits, losses=losses, total=total, dlogits=dl, dy2=dy2, dy1=dy1,
              dhs=dhs, dnorm=dnorm)
    k = _check_head(w, hl, t3, P, w2, valid.cpu(), targets, nb, weights, NL, fused=False)
    _check_head_wgrads(w, st, k, NL, fused=False)
    # decoder.norm's parameter gradients of the launched path: all rows in one reduction (workgroup partials of 4 rows, then the
    # grouped sum: <= rows + 4 additions, + 4 roundings of x-hat and the product)
    b = R.head_backward(P, dict(t3=c64(t3), hstats=(k["hmean"], k["hrstd"]), y1=k["y1"], y2=k["y2"]), k["dlogits"].reshape(-1, 4), w2,
                        snap=lambda n, v_: k[n])
    hold(w, "G norm", st.G[vt + "decoder.norm.weight"], b["dgamma_rows"].sum(0), rowsum_bound(b["dgamma_rows"], 8))
    hold(w, "G norm", st.G[vt + "decoder.norm.bias"], b["dbeta_rows"].sum(0), rowsum_bound(b["dbeta_rows"], 4))
    print(w.line(f"launched head B={B} P={Pn}"))


# ================================================================================================ (b) rt_qenc_fwd / rt_qenc_bwd
def _qenc_inputs(B, Lq, Pn, HW=20, seed=0):
    """Random memory, phrase halves and a context mask whose B * Pn rows cycle through three kinds: random, every token but one
    masked, nothing masked.  A case with fewer than three rows cannot hold them all: (2, 12, 1, 1) has a random row and a one-key
    row and no unmasked one; every other case holds all three."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    S = Lq + HW
    mem32 = torch.randn(B * S, E, device="cuda", generator=g)
    mem16 = mem32.to(torch.bfloat16)
    ctx = (torch.rand(B * Pn, Lq, device="cuda", generator=g) < 0.4).to(torch.uint8)
    ctx[:, 0] = 0                                        # random rows keep at least the CLS token
    ctx[1::3] = 1; ctx[1::3, Lq - 1] = 0                 # every token but one masked: a softmax over one key (the last token)
    ctx[2::3] = 0                                        # nothing masked
    cat16 = (0.5 * torch.randn(B * Pn, 2 * E, device="cuda", generator=g)).to(torch.bfloat16)
    return mem32, mem16, ctx.view(B, Pn, Lq).contiguous(), cat16, S


def _keep(fq, N):
    from test_gemm_gpu import hash_keep
    p, seed = fq["st1"][2:4]
    if not p > 0:
        return None, 0.0
    idx = np.arange(N * E, dtype=np.uint64)              # the site's element index: row * E + col
    return torch.from_numpy(hash_keep(seed, idx, p)).view(N, E), float(np.float32(p))


def _check_qenc_fwd(w, model, o, mem32, mem16, ctx, cat16_in, B, S, Lq, Pn, nq):
    P = params64(model)
    N = B * Pn
    fq = o["fq_ctx"]
    k = {n: c64(v) for n, v in o.items() if torch.is_tensor(v)}
    k.update(t1=c64(fq["t1"]), a16=c64(fq["a16"]), t2=c64(fq["t2"]), m1=c64(fq["st1"][0]), r1=c64(fq["st1"][1]), m2=c64(fq["st2"][0]),
             r2=c64(fq["st2"][1]), cat16=c64(fq["x16"]))
    m16 = c64(mem16).view(B, S, E)
    lang, cls32 = m16[:, :Lq], c64(mem32).view(B, S, E)[:, 0]
    phrase = c64(cat16_in)[:, E:].reshape(B, Pn, E)
    assert torch.equal(k["cat16"][:, E:], c64(cat16_in)[:, E:])             # the phrase half is not this launch's to touch
    keep, p = _keep(fq, N)
    # copies
    hold(w, "cls16", o["cls16"], m16[:, 0], 0.0)
    hold(w, "lang16", o["lang16"], lang.reshape(B * Lq, E), 0.0)
    shaped = dict(kq=(B, E), qs=(B, Lq, E), vs=(B, Lq, E), qw=(B, Pn, Lq), c16=(B, Pn, E), co=(B, Pn, E), t1=(N, E), a16=(N, E), t2=(N, E),
                  tgt32=(N * nq, E), qpos=(N * nq, E))
    kk = {n: k[n].reshape(s) for n, s in shaped.items()}
    kk["cat_left"] = k["cat16"][:, :E].reshape(B, Pn, E)
    f = R.qenc_forward(P, lang, cls32, phrase, ctx.cpu().bool(), nq, keep, p, snap=lambda n, v: kk[n])
    W = lambda n: (P[QE + n + "weight"], P[QE + n + "bias"])        # noqa: E731
    hold(w, "kq", o["kq"], f["kq"], pbound(lang[:, 0], *W("linear1.")))
    hold(w, "qs", o["qs"], f["qs"], pbound(lang, *W("linear2.")))
    hold(w, "vs", o["vs"], f["vs"], pbound(lang, *W("linear3.")))
    # softmax weights: the scores' product bound d s through the softmax, then the row gate
    ds = (E + 2) * U32 * torch.einsum("be,ble->bl", kk["kq"].abs(), kk["qs"].abs())[:, None, :].expand(B, Pn, Lq)
    slack = f["qw"] * (ds + (f["qw"] * ds).sum(-1, keepdim=True))
    hold_rows(w, "qw", o["qw"], f["qw"], 1e-5, slack=slack)
    masked = ctx.cpu().bool()
    assert float(kk["qw"][masked].abs().sum()) == 0.0                       # a masked token weighs exactly nothing
    cb = (Lq + 2) * U32 * torch.einsum("bpl,ble->bpe", kk["qw"].abs(), kk["vs"].abs())
    hold(w, "c16", o["c16"], f["c"], cb + U16 * f["c"].abs())
    hold(w, "co", o["co"], f["co"], pbound(kk["c16"], *W("context_out.0.")))
    for nm_m, nm_r, x in (("cmean", "crstd", kk["co"].reshape(N, E)), ("m1", "r1", kk["t1"]), ("m2", "r2", kk["t2"])):
        mean, rstd = R.ln_stats(x)
        bm, br = stat_bounds(x)
        hold(w, "ln mean", k[nm_m], mean, bm)
        hold(w, "ln rstd", k[nm_r], rstd, br)
    hold_rows(w, "cat16[:, :E]", kk["cat_left"], f["cat_left"], 1e-5, slack=U16 * f["cat_left"].abs())
    hold(w, "t1", fq["t1"], f["t1"], pbound(k["cat16"], *W("fuse_encoder_query.0.")))
    hold_rows(w, "a16", fq["a16"], f["a"], 1e-5, slack=U16 * f["a"].abs())
    if keep is not None:
        assert float(kk["a16"][~keep].abs().sum()) == 0.0                   # the mask itself: dropped elements are exactly zero ...
        live = keep & (f["y1"] > 1e-3 * f["y1"].abs().max())
        assert bool((kk["a16"][live] > 0).all())                            # ... and kept ones are there
        assert 0.02 < float((~keep).double().mean()) < 0.25
    hold(w, "t2", fq["t2"], f["t2"], pbound(kk["a16"], *W("fuse_encoder_query.4.")))
    hold_rows(w, "tgt32", o["tgt32"], f["tgt"], 1e-5)
    hold_rows(w, "qpos", o["qpos"], f["qpos"], 1e-5)
    hold(w, "tgt16", o["tgt16"], kk["tgt32"], U16 * kk["tgt32"].abs())
    hold(w, "tgtq16", o["tgtq16"], f["tgtq"], (U32 + U16) * f["tgtq"].abs())
    return k, kk, P, keep, p


QENC_CASES = [(2, 12, 1, 1, False), (1, 7, 3, 1, False), (3, 96, 5, 1, True), (2, 90, 16, 1, True), (8, 40, 1, 1, True), (2, 12, 3, 2, True)]


@pytest.mark.parametrize("B,Lq,Pn,nq,train", QENC_CASES)
def test_qenc_forward_stages_against_float64(hip, B, Lq, Pn, nq, train):
    """Every tensor rt_qenc_fwd stores, stage by stage; at two shapes the launched chain through the same checks."""
    model, crit, ocfg = _model(nq)
    model.train(train)
    net = model.net
    mem32, mem16, ctx, cat16, S = _qenc_inputs(B, Lq, Pn, seed=B + Lq)
    hip.set_seed_dev(None)                                # the dropout site is the plain seed
    try:
        modes = ("fused", "chain") if (B, Lq, Pn) in ((3, 96, 5), (2, 12, 3)) else ("fused",)
        for mode in modes:
            net.begin_step(train)
            cat = cat16.clone()
            if mode == "fused":
                assert model._qfuse_ok(Lq, Pn)
                o = model._qenc_fwd_fused(mem16, mem32, ctx, cat, B, S, Lq, Pn)
            else:
                qmask = torch.zeros(B, Pn, dtype=torch.uint8, device="cuda")
                r = model._qenc_fwd_chain(mem16, mem32, ctx, cat, cat.view(2 * B * Pn, -1), qmask, B, S, Lq, Pn)
                names = ("cls16", "lang16", "kq", "qs", "vs", "qw", "c16", "co", "cmean", "crstd", "fq_ctx", "tgt32", "tgt16", "qpos", "tgtq16")
                o = dict(zip(names, r[:15]))
            torch.cuda.synchronize()
            assert o["fq_ctx"]["st1"][2] == (0.1 if train else 0.0)
            w = Worst()
            _check_qenc_fwd(w, model, o, mem32, mem16, ctx, cat16, B, S, Lq, Pn, nq)
            print(w.line(f"qenc fwd {mode} B={B} L={Lq} P={Pn} nq={nq} train={train}"))
    finally:
        model.eval()


# rt_qenc_bwd is built for one query per phrase (it has no n_q): with two the model runs the launched chain, so that is what the
# (2, 12, 3, 2, True) case goes through, with and without gb
QENC_BWD_CASES = [c + (gb, "fused") for c in QENC_CASES if c[3] == 1 for gb in (False, True)] + [
    (3, 96, 5, 1, True, True, "chain"), (2, 12, 1, 1, False, False, "chain"), (2, 12, 3, 2, True, True, "chain"),
    (2, 12, 3, 2, True, False, "chain")]


@pytest.mark.parametrize("B,Lq,Pn,nq,train,with_gb,mode", QENC_BWD_CASES)
def test_qenc_backward_stages_against_float64(hip, monkeypatch, B, Lq, Pn, nq, train, with_gb, mode):
    """Every tensor rt_qenc_bwd stores, d query_embed, d memory per row class and the weight gradients behind it; the launched
    chain (its Linears' dy operands and results, caught at net.lin_bwd) through the same checks at two shapes with one query per
    phrase and at the two-query shape, where the upstream gradients have one row per (phrase, query): d query_embed [n_q, 2E] sums
    over the phrases, d fused over the queries."""
    model, crit, ocfg = _model(nq)
    model.train(train)
    net, st = model.net, model.store
    N = B * Pn                  # phrase rows; the upstream gradients have N * nq query rows
    assert model.cfg.n_q == nq and (nq == 1 or mode == "chain")
    mem32, mem16, ctx, cat16, S = _qenc_inputs(B, Lq, Pn, seed=100 + B + Lq)
    hip.set_seed_dev(None)
    cap = {}
    orig = hip.qenc_bwd
    monkeypatch.setattr(hip, "qenc_bwd", lambda **kw: (cap.update(kw), orig(**kw))[1])
    fused = mode == "fused"
    seen = {}
    lin_bwd = model.net.lin_bwd

    def lin_bwd_seen(key, dy, x, *a, **kw):
        r = lin_bwd(key, dy, x, *a, **kw)
        seen[key] = (dy, r[1])
        return r
    try:
        net.begin_step(train)
        o = model._qenc_fwd_fused(mem16, mem32, ctx, cat16, B, S, Lq, Pn)
        sv = dict(Nf=N, fq_ctx=o["fq_ctx"], co=o["co"], cst=(o["cmean"], o["crstd"]), c16=o["c16"], cls16=o["cls16"], lang16=o["lang16"],
                  kq=o["kq"], qs=o["qs"], vs=o["vs"], qw=o["qw"])
        g = torch.Generator(device="cuda").manual_seed(5)
        ga = torch.randn(N * nq, E, device="cuda", generator=g) * 1e-2
        gb = torch.randn(N * nq, E, device="cuda", generator=g) * 1e-2 if with_gb else None
        dqpos = torch.randn(N * nq, E, device="cuda", generator=g) * 1e-2
        dmem0 = torch.randn(B * S, E, device="cuda", generator=g) * 1e-2
        st.flat_g.zero_()
        gq = st.G[QE + "query_embed.weight"]
        gq.copy_(torch.randn(gq.shape, device="cuda", generator=g) * 1e-2)          # it is accumulated: start from something
        gq0 = c64(gq)
        dmem = dmem0.clone()
        if fused:
            dcat = model._qenc_bwd_fused(sv, ga, gb, dqpos, dmem, B, S, Lq, Pn)
        else:
            net.lin_bwd = lin_bwd_seen
            dcat, _ = model._qenc_bwd_chain(sv, ga, gb, dqpos, dmem, B, S, Lq, Pn, N * nq)
            fq, pq = o["fq_ctx"], lambda n: st.P[QE + n]        # noqa: E731
            cap.update(ga=ga, gb=gb, dqpos=dqpos, t2=fq["t2"], m2=fq["st2"][0], r2=fq["st2"][1], g5=pq("fuse_encoder_query.5.weight"),
                       bet5=pq("fuse_encoder_query.5.bias"), t1=fq["t1"], m1=fq["st1"][0], r1=fq["st1"][1], g1=pq("fuse_encoder_query.1.weight"),
                       bet1=pq("fuse_encoder_query.1.bias"), co=o["co"], cmean=o["cmean"], crstd=o["crstd"], kq=o["kq"], qs=o["qs"], vs=o["vs"],
                       qw=o["qw"])
            for nm_dy, nm_out, key in (("dt2b", "da", "fuse_encoder_query.4."), ("dt1b", "dcat", "fuse_encoder_query.0."),
                                       ("dcob", "dc", "context_out.0."), ("dk16", None, "linear1."), ("dqs16", None, "linear2."),
                                       ("dvs16", None, "linear3.")):
                cap[nm_dy] = seen[QE + key][0]
                if nm_out:
                    cap[nm_out] = seen[QE + key][1]
        net.flush_wgrads()
        torch.cuda.synchronize()
    finally:
        model.eval()
        net.__dict__.pop("lin_bwd", None)
    w = Worst()
    P = params64(model)
    fq = o["fq_ctx"]
    keep, p = _keep(fq, N)
    k = {n: c64(v) for n, v in cap.items() if torch.is_tensor(v)}
    assert dcat.data_ptr() == cap["dcat"].data_ptr()
    gate5 = ln_sign_f32(cap["t2"], cap["m2"], cap["r2"], cap["g5"], cap["bet5"])
    gate1 = ln_sign_f32(cap["t1"], cap["m1"], cap["r1"], cap["g1"], cap["bet1"])
    assert torch.equal(gate1 & (keep if keep is not None else gate1), c64(fq["a16"]) != 0)     # the stored activation says the same
    sv64 = dict(kq=k["kq"], qs=k["qs"].view(B, Lq, E), vs=k["vs"].view(B, Lq, E), qw=k["qw"], co=k["co"].view(B, Pn, E), t1=k["t1"], t2=k["t2"],
                st2=(k["m2"], k["r2"]), st1=(k["m1"], k["r1"]), cst=(k["cmean"].view(B, Pn), k["crstd"].view(B, Pn)))
    shaped = dict(dt2b=(N, E), da=(N, E), dt1b=(N, E), dcat=(N, 2 * E), dcob=(B, Pn, E), dc=(B, Pn, E), dk16=(B, E), dqs16=(B, Lq, E), dvs16=(B, Lq, E))
    kk = {n: k[n].reshape(s) for n, s in shaped.items()}
    b = R.qenc_backward(P, sv64, k["ga"], k.get("gb"), k["dqpos"], nq, gate5.double(), gate1.double(), keep, p, snap=lambda n, v: kk[n])
    Wn = lambda n: P[QE + n + "weight"]        # noqa: E731
    hold_rows(w, "dt2b", cap["dt2b"], b["dt2"], 2e-5, slack=U16 * b["dt2"].abs())
    hold(w, "da", cap["da"], b["da"], pbound(kk["dt2b"], Wn("fuse_encoder_query.4.").t()))
    hold_rows(w, "dt1b", cap["dt1b"], b["dt1"], 2e-5, slack=U16 * b["dt1"].abs())
    hold(w, "dcat", cap["dcat"], b["dcat"], pbound(kk["dt1b"], Wn("fuse_encoder_query.0.").t()))
    hold_rows(w, "dcob", cap["dcob"], b["dco"], 2e-5, slack=U16 * b["dco"].abs())
    hold(w, "dc", cap["dc"], b["dc"], pbound(kk["dcob"], Wn("context_out.0.").t()))
    # attention backward: dw = dc . v_l carries a product bound; d s = qw (dw - sum qw dw) cancels, so dw's bound goes through it
    # (and through the fp32 product / difference: 4 u of the operands) into d q_l = sum_j ds k and d k = sum_j sum_l ds q_l
    qw, vs_, qs_, kq_ = sv64["qw"], sv64["vs"], sv64["qs"], sv64["kq"]
    dw = torch.einsum("bpe,ble->bpl", kk["dc"], vs_)
    ddw = (E + 2) * U32 * torch.einsum("bpe,ble->bpl", kk["dc"].abs(), vs_.abs())
    dds = qw * (ddw + (qw * ddw).sum(-1, keepdim=True) + (Lq + 4) * U32 * (dw.abs() + (qw * dw.abs()).sum(-1, keepdim=True)))
    dds = torch.where(qw == 1.0, torch.zeros_like(dds), dds)                # one key: dw - dw is exactly zero in fp32 too
    hold_rows(w, "dk16", cap["dk16"], b["dk"], 1e-4, slack=U16 * b["dk"].abs() + torch.einsum("bpl,ble->be", dds, qs_.abs()))
    hold_rows(w, "dqs16", cap["dqs16"], b["dqs"], 1e-4, slack=U16 * b["dqs"].abs() + torch.einsum("bpl,be->ble", dds, kq_.abs()))
    hold_rows(w, "dvs16", cap["dvs16"], b["dvs"], 1e-4, slack=U16 * b["dvs"].abs())
    # the three LayerNorms' partial sums: one row pair per image over its P rows (<= P + 16 additions, + 4 roundings of x-hat and the product)
    # (d fused = sum over the phrase's queries of ga (+ gb) + d query_pos is itself an fp32 sum of up to 3 n_q pieces that can cancel:
    # pa = 3 n_q - 1 more roundings, measured against the pieces' magnitudes)
    pa = 3 * nq - 1
    d5 = b["df"] * gate5
    pieces = k["ga"].abs() + (k["gb"].abs() if with_gb else 0) + k["dqpos"].abs()          # per query row
    m5 = pieces.view(N, nq, E).sum(1) * gate5                                               # d fused also sums the queries of a phrase
    for nm, pfx, dy, x, stt, mag in (("part5", "fuse_encoder_query.5.", d5, k["t2"], sv64["st2"], m5),
                                     ("part1", "fuse_encoder_query.1.", b["dy1"], k["t1"], sv64["st1"], None),
                                     ("partc", "context_out.1.", kk["dcat"][:, :E], k["co"], (k["cmean"], k["crstd"]), None)):
        gr, br_ = R.ln_param_rows(dy, x, stt)
        mg, mb = (None, None) if mag is None else R.ln_param_rows(mag, x, stt)
        if not fused:       # rt_layernorm_bwd: workgroup partials of 4 rows, then the grouped sum: <= rows + 16 additions
            hold(w, "G ln", st.G[QE + pfx + "weight"], gr.sum(0), rowsum_bound(gr, 16 + 4 + pa, None if mg is None else mg.abs()))
            hold(w, "G ln", st.G[QE + pfx + "bias"], br_.sum(0), rowsum_bound(br_, 16 + pa, None if mb is None else mb.abs()))
            continue
        for bi in range(B):
            rows = slice(bi * Pn, (bi + 1) * Pn)
            hold(w, nm, cap[nm][bi, 0], gr[rows].sum(0), rowsum_bound(gr[rows], 16 + 4 + pa, None if mg is None else mg[rows].abs()))
            hold(w, nm, cap[nm][bi, 1], br_[rows].sum(0), rowsum_bound(br_[rows], 16 + pa, None if mb is None else mb[rows].abs()))
    # d query_embed [n_q, 2E]: accumulated on what is there, with atomics per wave (one launch), one column sum per upstream piece
    # (the chain, one query) or ga + gb summed over the phrases and added (the chain, more queries): at most 2 N + 4 additions per
    # query, measured against the pieces' magnitudes
    dt = (k["ga"] + (k["gb"] if with_gb else 0)).view(N, nq, E)
    dta = (k["ga"].abs() + (k["gb"].abs() if with_gb else 0)).view(N, nq, E)
    dqp = k["dqpos"].view(N, nq, E)
    assert tuple(gq0.shape) == (nq, 2 * E)
    for qi in range(nq):
        terms = torch.cat([gq0[qi].view(1, 2 * E), torch.cat([dt[:, qi], dqp[:, qi]], dim=-1)])
        mags = torch.cat([gq0[qi].view(1, 2 * E).abs(), torch.cat([dta[:, qi], dqp[:, qi].abs()], dim=-1)])
        hold(w, "dqembed", st.G[QE + "query_embed.weight"][qi], terms.sum(0), rowsum_bound(terms, N + 4, mags))
    # d memory per row class
    dm, dm0 = c64(dmem).view(B, S, E), c64(dmem0).view(B, S, E)
    assert torch.equal(dm[:, Lq:], dm0[:, Lq:])                               # image rows: not this launch's
    W1, W2, W3 = Wn("linear1."), Wn("linear2."), Wn("linear3.")
    lang = dm0[:, :Lq] + b["dlang"]
    labs = dm0[:, :Lq].abs() + kk["dqs16"].abs() @ W2.abs() + kk["dvs16"].abs() @ W3.abs()
    hold(w, "dmem lang", dm[:, 1:Lq], lang[:, 1:], (2 * E + 8) * U32 * labs[:, 1:])
    cls = lang[:, 0] + b["dcls_res"] + b["dcls_lin"]
    cabs = labs[:, 0] + kk["dcat"][:, :E].reshape(B, Pn, E).abs().sum(1) + kk["dk16"].abs() @ W1.abs()
    hold(w, "dmem cls", dm[:, 0], cls, (3 * E + Pn + 10) * U32 * cabs)
    # weight / bias gradients from the kernel's own dy tensors
    for name, dy, x in (("fuse_encoder_query.4.", kk["dt2b"], c64(fq["a16"])), ("fuse_encoder_query.0.", kk["dt1b"], c64(fq["x16"])),
                        ("context_out.0.", kk["dcob"].reshape(N, E), c64(o["c16"])), ("linear1.", kk["dk16"], c64(o["cls16"])),
                        ("linear2.", kk["dqs16"].reshape(-1, E), c64(o["lang16"])), ("linear3.", kk["dvs16"].reshape(-1, E), c64(o["lang16"]))):
        rows = dy.shape[0]
        hold(w, "G weight", st.G[QE + name + "weight"], dy.t() @ x, (rows + 2) * U32 * (dy.abs().t() @ x.abs()))
        hold(w, "G bias", st.G[QE + name + "bias"], dy.sum(0), rowsum_bound(dy, 2))
    for nm, pfx in (("part5", "fuse_encoder_query.5."), ("part1", "fuse_encoder_query.1."), ("partc", "context_out.1.")) if fused else ():
        pt = c64(cap[nm])
        hold(w, "G ln", st.G[QE + pfx + "weight"], pt[:, 0].sum(0), rowsum_bound(pt[:, 0], 2))
        hold(w, "G ln", st.G[QE + pfx + "bias"], pt[:, 1].sum(0), rowsum_bound(pt[:, 1], 2))
    print(w.line(f"qenc bwd {mode} B={B} L={Lq} P={Pn} nq={nq} train={train} gb={with_gb}"))


# ================================================================================================ (c) decoder forward
DEC_CASES = {"single-B2": ("e2e_single", 2, 96, 128, 0), "single-B13": ("e2e_single", 13, 64, 64, 0), "multi-B2": ("e2e_multi", 2, 96, 128, 3)}
NH = 8


@functools.lru_cache(maxsize=None)
def _decoder_run(case):
    """The whole small model's forward in eval mode; what it saved for the backward, and the query encoder's outputs (the stack's
    fp32 input and query_pos, which the backward does not need and the model therefore does not keep)."""
    from reftr_amd.util.misc import NestedTensor
    model, crit, ocfg = _model(1)
    name, B, H, W, n_phrase = DEC_CASES[case]
    samples, _ = make_inputs(name, B=B, H=H, W=W, L=12, n_phrase=n_phrase)
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].cuda(), samples["img_mask"].cuda())
    cap = {}
    orig = model._qenc_fwd_fused
    model._qenc_fwd_fused = lambda *a, **k: cap.setdefault("q", orig(*a, **k))
    try:
        model.eval()
        model(s)
    finally:
        del model._qenc_fwd_fused
    torch.cuda.synchronize()
    sv = model._saved
    coop = [bool(r.get("coop")) for r in sv["dec"]]
    assert all(coop) if n_phrase == 0 else not any(coop), (case, coop)          # which path ran
    if n_phrase:
        assert int(sv["qmask"].sum()) > 0                                         # at least one padded phrase
    return sv, cap["q"]


def _dec_tensors(sv, q):
    B, S, T, N = sv["B"], sv["S"], sv["T"], sv["N"]
    v3 = lambda x, rows: c64(x).view(B, rows, -1)        # noqa: E731
    d = dict(tgt32=v3(q["tgt32"], T), qpos=v3(q["qpos"], T), tgt16=v3(q["tgt16"], T), tgtq16=v3(q["tgtq16"], T), mem16=v3(sv["mem16"], S),
             memp16=v3(sv["memp16"], S), kpm=sv["kpm"].cpu().bool().view(B, S), qmask=sv["qmask"].cpu().bool().view(B, T),
             t3=c64(sv["t3s"]).view(-1, B, T, E))
    layers = []
    for r in sv["dec"]:
        kk = {n: v3(r[n], S if n in ("k2", "v2") else T) for n in ("o", "u", "t1q16", "q2", "k2", "v2", "o2", "u2", "t2_16", "hdn", "u3")}
        if T > 1:
            kk.update(qk=v3(r["qk"], T), v=v3(r["v"], T))
        layers.append(kk)
    return d, layers


def _score_bound(q, k, mask):
    """(dh + 3) u scale |q| |k|^T per head (the scaled product of dh terms), zero at masked keys; [B, H, Tq, Tk]"""
    B, Tq, _ = q.shape
    dh = E // NH
    hd = lambda x: x.abs().view(B, -1, NH, dh).transpose(1, 2)        # noqa: E731
    ds = (dh + 3) * U32 * dh ** -0.5 * (hd(q) @ hd(k).transpose(-1, -2))
    return ds if mask is None else ds.masked_fill(mask[:, None, None, :], 0.0)


@pytest.mark.parametrize("case", list(DEC_CASES))
def test_decoder_forward_stages_against_float64(hip, case):
    """Every tensor every decoder layer saves (eval mode; dropout-on runs stay with the bit-identity tests of
    tests/test_decoder_coop_gpu.py): the cooperative launch on the single-phrase cases, the launched chain with the real
    self-attention and the query padding mask on the multi-phrase one."""
    model, crit, ocfg = _model(1)
    sv, q = _decoder_run(case)
    B, S, T = sv["B"], sv["S"], sv["T"]
    P = params64(model)
    d, layers = _dec_tensors(sv, q)
    dh, scale = E // NH, (E // NH) ** -0.5
    hd = lambda x: x.view(B, -1, NH, dh).transpose(1, 2)        # noqa: E731
    w = Worst()
    t32, t16, tq16 = d["tgt32"], d["tgt16"], d["tgtq16"]
    for i, (r, kk) in enumerate(zip(sv["dec"], layers)):
        p = f"{VT}decoder.layers.{i}."
        assert torch.equal(c64(r["t16"]).view(B, T, E), t16)
        f = R.decoder_layer(P, p, t32, t16, tq16, d["qpos"], d["mem16"], d["memp16"], d["qmask"], d["kpm"], NH, snap=lambda n, v: kk.get(n, v))
        Wi, bi = P[p + "self_attn.in_proj_weight"], P[p + "self_attn.in_proj_bias"]
        Wc, bc = P[p + "multihead_attn.in_proj_weight"], P[p + "multihead_attn.in_proj_bias"]
        Wb = lambda n: (P[p + n + "weight"], P[p + n + "bias"])        # noqa: E731
        if T > 1:
            hold(w, "sa v", r["v"], f["v"], pbound(t16, Wi[2 * E:], bi[2 * E:]) + U16 * f["v"].abs())
            hold(w, "sa qk", r["qk"], f["qk"], pbound(tq16, Wi[:2 * E], bi[:2 * E]) + U16 * f["qk"].abs())
            # rt_attn_fwd hands the probabilities to the P V product as bf16 operands: test_attention_fwd_bwd's gate, per (image, query)
            hold_rows(w, "sa o", r["o"], f["o"], 4e-3)
            dsc = _score_bound(kk["qk"][..., :E], kk["qk"][..., E:], d["qmask"])
            hold(w, "sa lse", r["lse"], f["lse"], dsc.amax(-1) + 1e-5 * f["lse"].abs())
        else:
            hold(w, "sa o", r["o"], f["o"], pbound(t16, Wi[2 * E:], bi[2 * E:]) + U16 * f["o"].abs())
        Wo, bo = Wb("self_attn.out_proj.")
        hold(w, "u", r["u"], f["u"], (E + 3) * U32 * (kk["o"].abs() @ Wo.abs().t() + bo.abs() + t32.abs()))
        for j, nm in ((1, "u"), (2, "u2"), (3, "u3")):
            mean, rstd = R.ln_stats(kk[nm])
            bm, br = stat_bounds(kk[nm])
            hold(w, "ln mean", r[f"st{j}"][0], mean, bm)
            hold(w, "ln rstd", r[f"st{j}"][1], rstd, br)
        hold_rows(w, "t1q16", r["t1q16"], f["t1q"], 1e-5, slack=U16 * f["t1q"].abs())
        hold(w, "q2", r["q2"], f["q2"], pbound(kk["t1q16"], Wc[:E], bc[:E]) + U16 * f["q2"].abs())
        hold(w, "k2", r["k2"], f["k2"], pbound(d["memp16"], Wc[E:2 * E], bc[E:2 * E]) + U16 * f["k2"].abs())
        hold(w, "v2", r["v2"], f["v2"], pbound(d["mem16"], Wc[2 * E:], bc[2 * E:]) + U16 * f["v2"].abs())
        # cross-attention: the scores' product bound through the softmax into P V, the P V sum's own bound, the bf16 store; what is
        # left is held by the attention-stage gate per (image, query) row (one query: fp32 probabilities, the softmax gate; more:
        # bf16 probabilities inside rt_attn_fwd, test_attention_fwd_bwd's gate)
        dsc = _score_bound(kk["q2"], kk["k2"], d["kpm"])
        _, _, pr = R.attention(kk["q2"], kk["k2"], kk["v2"], d["kpm"], NH, scale)
        dp = pr * (dsc + (pr * dsc).sum(-1, keepdim=True))
        va = hd(kk["v2"].abs())
        slack = ((dp @ va) + (S + 2) * U32 * (pr @ va)).transpose(1, 2).reshape(B, T, E) + U16 * f["o2"].abs()
        hold_rows(w, "o2", r["o2"], f["o2"], 1e-5 if T == 1 else 4e-3, slack=slack)
        hold(w, "lse2", r["lse2"], f["lse2"], dsc.amax(-1) + 1e-5 * f["lse2"].abs())
        # u2 / u3 add the fp32 LayerNorm output the kernels keep in registers (not stored): the product's bound, then the LayerNorm
        # gate on that row
        Wo2, bo2 = Wb("multihead_attn.out_proj.")
        hold_rows(w, "u2", r["u2"], f["u2"], 1e-5, slack=(E + 3) * U32 * (kk["o2"].abs() @ Wo2.abs().t() + bo2.abs() + f["t1"].abs()), scale=f["t1"])
        hold_rows(w, "t2_16", r["t2_16"], f["t2"], 1e-5, slack=U16 * f["t2"].abs())
        hold(w, "hdn", r["hdn"], f["hdn"], pbound(kk["t2_16"], *Wb("linear1.")) + U16 * f["hdn"].abs())
        W2, b2 = Wb("linear2.")
        F_ = W2.shape[1]
        hold_rows(w, "u3", r["u3"], f["u3"], 1e-5, slack=(F_ + 3) * U32 * (kk["hdn"].abs() @ W2.abs().t() + b2.abs() + f["t2"].abs()), scale=f["t2"])
        hold_rows(w, "t3", d["t3"][i], f["t3"], 1e-5)
        t32 = d["t3"][i]
        if i + 1 < len(layers):
            nxt = sv["dec"][i + 1]
            t16 = c64(nxt["t16"]).view(B, T, E)
            hold(w, "t3_16", t16, t32, U16 * t32.abs())
            if T > 1:           # the real self-attention reads it; the one-key form (folded into its value product) has none
                tq16 = c64(nxt["tq16"]).view(B, T, E)
                hold(w, "t3q16", tq16, t32 + d["qpos"], (U32 + U16) * (t32 + d["qpos"]).abs())
    print(w.line(f"decoder fwd {case} ({'cooperative' if sv['dec'][0].get('coop') else 'launched chain'})"))


# ================================================================================================ (d) decoder backward
class _Through(torch.autograd.Function):
    """Going forward: the kernel's stored tensor.  Coming back: the gradient passes (rounded to bf16 on request).  The reference is
    linearised at the kernel's own forward."""

    @staticmethod
    def forward(ctx, x, val, rnd):
        ctx.rnd = rnd
        return val.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.to(torch.bfloat16).double() if ctx.rnd else g), None, None


# gradients the backward kernels hand on as bf16 operands (dec_layer_bwd / rt_decoder_bwd): d o (= d v of the folded self-attention),
# d hdn, d o2, d q2, d k2, d v2, with real self-attention also d qk and d v; and, through `gq`, d u / d u2 / d u3 on their way into
# out_proj / linear2 (du_b, du2_b, du3_b: the LayerNorm backward's bf16 copy; the residual keeps the fp32 one).  The gradients of
# t16 / t1q16 / t2_16 stay fp32 (out_f32 products).
G_ROUNDED = ("o", "hdn", "o2", "q2", "k2", "v2", "qk", "v")


class _AttnDeltaFromStoredO(torch.autograd.Function):
    """R.attention with the backward the attention kernels run (rt_attn_bwd's row_delta, rt_decoder_bwd's B6): the softmax
    backward's row term sum_k p_k dp_k = dO . O is taken from the STORED output, which is bf16 -- a rounding point of the backward
    that is no gradient rounding (d s = p (dp - delta) cancels, so delta's 2^-9 moves every key's d s).  The rounded twin rounds
    its own P V to bf16 here; everything else is exact."""

    @staticmethod
    def forward(ctx, q, k, v, mask, H, scale):
        o, lse, p = R.attention(q, k, v, mask, H, scale)
        ctx.save_for_backward(q, k, v, p, o)
        ctx.H, ctx.scale = H, scale
        return o, lse, p

    @staticmethod
    def backward(ctx, do, dlse, dp_unused):
        q, k, v, p, o = ctx.saved_tensors
        B, Tq, E_ = q.shape
        hd = lambda x: x.view(B, -1, ctx.H, E_ // ctx.H).transpose(1, 2)        # noqa: E731
        un = lambda x: x.transpose(1, 2).reshape(B, -1, E_)        # noqa: E731
        doh = hd(do)
        delta = (doh * hd(o.to(torch.bfloat16).double())).sum(-1, keepdim=True)
        ds = p * (doh @ hd(v).transpose(-1, -2) - delta) * ctx.scale
        return un(ds @ hd(k)), un(ds.transpose(-1, -2) @ hd(q)), un(p.transpose(-1, -2) @ doh), None, None, None


def _twin_grads(P0, d, layers, dt3, rounded):
    B, T, _ = d["tgt32"].shape
    names = [k for k in P0 if k.startswith(VT + "decoder.layers.")]
    P = {k: P0[k].clone().requires_grad_(True) for k in names}
    leaves = dict(tgt=d["tgt32"].clone().requires_grad_(True), qpos=d["qpos"].clone().requires_grad_(True),
                  mem=d["mem16"].clone().requires_grad_(True), memp=d["memp16"].clone().requires_grad_(True))
    tgt, qpos = leaves["tgt"], leaves["qpos"]
    t32, t16, tq16 = tgt, _Through.apply(tgt, d["tgt16"], False), _Through.apply(tgt + qpos, d["tgtq16"], False)
    obj = 0.0
    for i, kk in enumerate(layers):
        snap = lambda n, v, kk=kk: _Through.apply(v, kk[n], rounded and n in G_ROUNDED) if n in kk else v        # noqa: E731
        gq = lambda n, y: _Through.apply(y, y.detach(), rounded)        # noqa: E731
        f = R.decoder_layer(P, f"{VT}decoder.layers.{i}.", t32, t16, tq16, qpos, leaves["mem"], leaves["memp"], d["qmask"], d["kpm"], NH,
                            snap=snap, gq=gq, hdn_gate=(kk["hdn"] != 0).double(), attn=_AttnDeltaFromStoredO.apply if rounded else None)
        obj = obj + (f["t3"] * dt3[i]).sum()
        t32 = _Through.apply(f["t3"], d["t3"][i], False)
        if i + 1 < len(layers):
            t16 = _Through.apply(f["t3"], (layers[i + 1]["t16"] if "t16" in layers[i + 1] else d["t3"][i]), False)
            tq16 = _Through.apply(f["t3"] + qpos, (layers[i + 1]["tq16"] if "tq16" in layers[i + 1] else d["t3"][i] + d["qpos"]), False)
    allv = {**leaves, **P}
    g = torch.autograd.grad(obj, list(allv.values()), allow_unused=True)
    return {k: (torch.zeros_like(allv[k]) if v is None else v) for k, v in zip(allv, g)}


@pytest.mark.parametrize("case", list(DEC_CASES))
def test_decoder_backward_against_the_float64_twin(hip, case):
    """rt_decoder_bwd (both memory-gradient forms) / the dec_layer_bwd loop on a fixed random d t3 of every layer, against float64
    autograd through the stage functions linearised at the kernel's forward.  The gate per tensor is 3 x the distance the twin
    itself moves when its gradients are rounded to bf16 where the kernels round them, + 1e-6, and never above 3e-2: d query_pos,
    whose floor is 1.1 - 1.8e-2 at these inputs (the stored-output delta of the attention backward, see _AttnDeltaFromStoredO: its
    error is the same for every key of a row, so it adds up coherently in d q = sum_k ds_k k_k), is held at 3e-2 = 1.6 - 2.7 x its
    floor instead of 3 x."""
    model, crit, ocfg = _model(1)
    net, st = model.net, model.store
    sv, q = _decoder_run(case)
    B, S, T, N, NL = sv["B"], sv["S"], sv["T"], sv["N"], sv["NL"]
    P = params64(model)
    d, layers = _dec_tensors(sv, q)
    for i, r in enumerate(sv["dec"]):       # the bf16 copies of a layer's output the next layer reads
        if i > 0:
            layers[i]["t16"] = c64(r["t16"]).view(B, T, E)
            if r.get("tq16") is not None:
                layers[i]["tq16"] = c64(r["tq16"]).view(B, T, E)
    g = torch.Generator(device="cuda").manual_seed(17)
    dt3_dev = torch.randn(NL * N, E, device="cuda", generator=g) * 1e-2
    dt3 = c64(dt3_dev).view(NL, B, T, E)
    exact = _twin_grads(P, d, layers, dt3, rounded=False)
    rnd = _twin_grads(P, d, layers, dt3, rounded=True)
    rel = lambda a, b_: float((a - b_).norm() / (b_.norm() + 1e-300))        # noqa: E731
    floor = {k: rel(rnd[k], exact[k]) for k in exact}
    prefixes = [f"{VT}decoder.layers.{i}." for i in range(NL)]
    coop = bool(sv["dec"][0].get("coop"))
    M = B * S
    rows = []
    packs = (True, False) if coop else (None,)
    try:
        for pack in packs:
            st.flat_g.zero_()
            zz = torch.zeros(2 * M + N, E, dtype=torch.float32, device="cuda")
            dmem, dmemp, dqpos = zz[:M], zz[M:2 * M], zz[2 * M:]
            if coop:
                net.dec_kv_pack = pack
                dtgt = net.dec_stack_bwd_coop(prefixes, sv["dec"], dt3_dev, sv["mem16"], sv["memp16"], sv["kpm"], B, S, dmem, dmemp, dqpos)
            else:
                ga = gb = None
                for i in reversed(range(NL)):
                    dn = dt3_dev[i * N:(i + 1) * N]
                    extra = None if ga is None else (ga if gb is None else ga + gb)
                    ga, gb = net.dec_layer_bwd(prefixes[i], sv["dec"][i], dn, extra, sv["mem16"], sv["memp16"], sv["qmask"], sv["kpm"],
                                               B, T, S, dmem, dmemp, dqpos)
                dtgt = ga if gb is None else ga + gb
            net.flush_wgrads()
            torch.cuda.synchronize()
            if coop:
                assert int(net.dec_counters[-1]) == 0, "a cooperative wait gave up"
            got = dict(tgt=c64(dtgt).view(B, T, E), qpos=c64(dqpos).view(B, T, E), mem=c64(dmem).view(B, S, E), memp=c64(dmemp).view(B, S, E))
            got.update({k: c64(st.G[k]) for k in exact if k.startswith(VT)})
            for k in exact:
                gate = min(3 * floor[k] + 1e-6, 3e-2)       # no gate above 3e-2, whatever the floor
                rows.append((pack, k, floor[k], rel(got[k].reshape(exact[k].shape), exact[k]), gate))
    finally:
        net.dec_kv_pack = True
    print(f"\n[decoder bwd {case}] {'kv_pack':8s} {'tensor':62s} {'floor':>9s} {'measured':>9s} {'gate':>9s}")
    for pack, k, fl, m, gt in rows:
        print(f"  {str(pack):8s} {k:62s} {fl:9.2e} {m:9.2e} {gt:9.2e}{'   <-- over' if m > gt else ''}")
    bad = [(pack, k, m, gt) for pack, k, fl, m, gt in rows if not m <= gt]
    assert not bad, bad
