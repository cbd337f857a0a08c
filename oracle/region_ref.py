"""float64 stage functions of the few-row region: query encoder -> decoder stack -> decoder.norm -> box head -> box losses,
forward and backward, written from the formulas (models/reftr_transformer.py:41-66, models/modeling/transformer.py:231-252,
models/modeling/backbone.py:26-38, models/criterion.py:113-153; reftr_oracle.query_encoder / decoder_layer / loss_boxes).

One small function per stage, each taking the stage's inputs and returning its output BEFORE any rounding.  The composed
forwards take a `snap(name, value)` hook that is called on every tensor a kernel stores: the identity composes the stages
free-running (tests/test_region_ref_cpu.py pins that composition to the oracle at 1e-10); a hook that returns the kernel's own
stored tensor makes every stage start from what the kernel itself read for it (tests/test_region_fp64_gpu.py), the value handed
to the hook being the reference for that stored tensor.

Layout is batch-major ([B, T, E]; the oracle is sequence-first).  Parameters come in a dict of float64 tensors under their
state-dict names.  Test infrastructure: nothing under reftr_amd/ imports this module.
"""
import torch

from . import reftr_oracle as O

EPS = 1e-5


def _id(name, x):
    return x


# ---------------------------------------------------------------------------------------------- building blocks
def lin(x, W, b=None):
    y = x @ W.transpose(-1, -2)
    return y if b is None else y + b


def ln_stats(x, eps=EPS):
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    return mean, (var + eps).rsqrt()


def ln(x, g, b, stats=None, eps=EPS):
    mean, rstd = ln_stats(x, eps) if stats is None else stats
    return (x - mean[..., None]) * rstd[..., None] * g + b


def ln_bwd(dy, x, g, stats=None, eps=EPS):
    """dx of y = LayerNorm(x) for the upstream dy (already through any ReLU / dropout gate)."""
    mean, rstd = ln_stats(x, eps) if stats is None else stats
    xh = (x - mean[..., None]) * rstd[..., None]
    gg = dy * g
    return rstd[..., None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))


def ln_param_rows(dy, x, stats=None, eps=EPS):
    """per-row contributions to (d gamma, d beta); the caller sums the rows it wants"""
    mean, rstd = ln_stats(x, eps) if stats is None else stats
    return dy * (x - mean[..., None]) * rstd[..., None], dy


def dropout(x, keep, p):
    return x if keep is None else x * keep / (1.0 - p)


# ---------------------------------------------------------------------------------------------- query encoder, forward
def qenc_scores(kq, qs):
    """kq [B, E], qs [B, L, E] -> k . q_l [B, L] (no 1 / sqrt(d))"""
    return torch.einsum("be,ble->bl", kq, qs)


def qenc_softmax(s, ctx):
    """s [B, L], ctx [B, P, L] (True = ignore) -> [B, P, L]"""
    return torch.softmax(s[:, None, :].expand(ctx.shape).masked_fill(ctx, float("-inf")), dim=-1)


def qenc_context(qw, vs):
    return torch.einsum("bpl,ble->bpe", qw, vs)


def qenc_split(f, qembed, nq):
    """f [N, E], query_embed [n_q, 2E] -> tgt, qpos, tgt + qpos, each [N * n_q, E], rows phrase-major (phrase, q)"""
    N, E = f.shape
    emb = qembed.view(nq, 2, E)
    tgt = (f[:, None, :] + emb[None, :, 0]).reshape(N * nq, E)
    qpos = (f[:, None, :] + emb[None, :, 1]).reshape(N * nq, E)
    return tgt, qpos, tgt + qpos


def qenc_forward(P, lang, cls32, phrase, ctx, nq, keep=None, p=0.0, snap=_id, pfx="query_encoder."):
    """lang [B, L, E]: the language rows of memory as the Linears read them (row 0 = CLS); cls32 [B, E]: the CLS row as the
    residual reads it; phrase [B, Pn, E]: map_phrase's output (right half of the concatenated row); ctx [B, Pn, L] True = ignore;
    keep [B * Pn, E] bool / None with drop probability p.  Returns every stage (the value before `snap`)."""
    B, Pn, E = phrase.shape
    N = B * Pn
    r = {}
    W = lambda n: (P[pfx + n + "weight"], P[pfx + n + "bias"])        # noqa: E731
    r["kq"] = lin(lang[:, 0], *W("linear1."))
    r["qs"] = lin(lang, *W("linear2."))
    r["vs"] = lin(lang, *W("linear3."))
    kq, qs, vs = snap("kq", r["kq"]), snap("qs", r["qs"]), snap("vs", r["vs"])
    r["s"] = qenc_scores(kq, qs)
    r["qw"] = qenc_softmax(r["s"], ctx)
    qw = snap("qw", r["qw"])
    r["c"] = qenc_context(qw, vs)
    c16 = snap("c16", r["c"])
    r["co"] = lin(c16, *W("context_out.0."))
    co = snap("co", r["co"])
    r["cn"] = ln(co, *W("context_out.1."))
    r["cat_left"] = r["cn"] + cls32[:, None, :]
    cat = torch.cat([snap("cat_left", r["cat_left"]), phrase], dim=-1).reshape(N, 2 * E)
    r["t1"] = lin(cat, *W("fuse_encoder_query.0."))
    t1 = snap("t1", r["t1"])
    r["y1"] = torch.relu(ln(t1, *W("fuse_encoder_query.1.")))
    r["a"] = dropout(r["y1"], keep, p)
    a16 = snap("a16", r["a"])
    r["t2"] = lin(a16, *W("fuse_encoder_query.4."))
    t2 = snap("t2", r["t2"])
    r["f"] = torch.relu(ln(t2, *W("fuse_encoder_query.5.")))
    r["tgt"], r["qpos"], _ = qenc_split(r["f"], P[pfx + "query_embed.weight"], nq)
    tgt, qpos = snap("tgt32", r["tgt"]), snap("qpos", r["qpos"])
    r["tgtq"] = tgt + qpos
    return r


# ---------------------------------------------------------------------------------------------- query encoder, backward
def qenc_split_bwd(ga, gb, dqpos, nq):
    """upstream of tgt (ga: direct, gb: through tgt + qpos, or None) and of qpos (dqpos, which already holds the tgt + qpos
    share) -> d fused [N, E], d query_embed [n_q, 2E]"""
    E = ga.shape[-1]
    dt = ga if gb is None else ga + gb
    df = (dt + dqpos).view(-1, nq, E).sum(1)
    return df, torch.cat([dt.view(-1, nq, E).sum(0), dqpos.view(-1, nq, E).sum(0)], dim=-1)


def qenc_attn_bwd(kq, qs, vs, qw, dc):
    """c = sum_l qw v_l, qw = softmax_l(k . q_l): dc [B, P, E] -> d kq [B, E], d qs [B, L, E], d vs [B, L, E]"""
    dw = torch.einsum("bpe,ble->bpl", dc, vs)
    ds = qw * (dw - (qw * dw).sum(-1, keepdim=True))
    return torch.einsum("bpl,ble->be", ds, qs), torch.einsum("bpl,be->ble", ds, kq), torch.einsum("bpl,bpe->ble", qw, dc)


def qenc_backward(P, sv, ga, gb, dqpos, nq, gate5, gate1, keep=None, p=0.0, snap=_id, pfx="query_encoder."):
    """The forward's stages transposed.  sv: the forward's tensors (kq, qs, vs, qw, co, t1, t2 as stored); gate5 / gate1: the ReLU
    gates of fuse_encoder_query.5 / .1 as tensors; keep / p: the dropout mask.  Returns every backward stage, the gradient of the
    language rows [B, L, E] (dlang; row 0 also takes dcls_res, the residual's share), and d query_embed."""
    B, L, E = sv["qs"].shape
    W = lambda n: P[pfx + n + "weight"]        # noqa: E731
    r = {}
    df, r["dqembed"] = qenc_split_bwd(ga, gb, dqpos, nq)
    r["df"] = df
    r["dt2"] = ln_bwd(df * gate5, sv["t2"], W("fuse_encoder_query.5."), sv.get("st2"))
    dt2b = snap("dt2b", r["dt2"])
    r["da"] = dt2b @ W("fuse_encoder_query.4.")
    da = snap("da", r["da"])
    r["dy1"] = dropout(da, keep, p) * gate1
    r["dt1"] = ln_bwd(r["dy1"], sv["t1"], W("fuse_encoder_query.1."), sv.get("st1"))
    dt1b = snap("dt1b", r["dt1"])
    r["dcat"] = dt1b @ W("fuse_encoder_query.0.")
    dcat = snap("dcat", r["dcat"])
    dleft = dcat[:, :E].reshape(B, -1, E)
    r["dco"] = ln_bwd(dleft, sv["co"], W("context_out.1."), sv.get("cst"))
    dcob = snap("dcob", r["dco"])
    r["dc"] = dcob @ W("context_out.0.")
    dc = snap("dc", r["dc"])
    r["dk"], r["dqs"], r["dvs"] = qenc_attn_bwd(sv["kq"], sv["qs"], sv["vs"], sv["qw"], dc)
    dk16, dqs16, dvs16 = snap("dk16", r["dk"]), snap("dqs16", r["dqs"]), snap("dvs16", r["dvs"])
    r["dcls_res"] = dleft.sum(1)
    r["dcls_lin"] = dk16 @ W("linear1.")
    r["dlang"] = dqs16 @ W("linear2.") + dvs16 @ W("linear3.")
    return r


# ---------------------------------------------------------------------------------------------- head
def head_forward(P, t3, snap=_id, norm="vl_transformer.decoder.norm.", mlp="bbox_embed.layers."):
    W = lambda n: (P[n + "weight"], P[n + "bias"])        # noqa: E731
    r = {}
    r["hs"] = ln(t3, *W(norm))
    hs16 = snap("hs16", r["hs"])
    r["y1"] = torch.relu(lin(hs16, *W(mlp + "0.")))
    y1 = snap("y1", r["y1"])
    r["y2"] = torch.relu(lin(y1, *W(mlp + "1.")))
    y2 = snap("y2", r["y2"])
    r["logits"] = lin(y2, *W(mlp + "2."))
    return r


def head_losses(logits, valid, targets, num_boxes, weights):
    """logits [NL, B, Pn, K, 4] (pre-sigmoid), valid [B, Pn * K] bool, targets [{'boxes': [n, 4]}], weights [NL, 2] = the layer's
    (bbox, giou) coefficients.  Returns losses [NL, 2], total = sum weights * losses, d total / d logits (float64 autograd
    through the oracle's loss_boxes / giou_diag)."""
    lg = logits.detach().clone().requires_grad_(True)
    rows = []
    for l in range(lg.shape[0]):
        d = O.loss_boxes(lg[l].sigmoid(), valid, targets, num_boxes)
        rows.append(torch.stack([d["loss_bbox"], d["loss_giou"]]))
    losses = torch.stack(rows)
    total = (losses * weights).sum()
    (dl,) = torch.autograd.grad(total, lg)
    return losses.detach(), total.detach(), dl


def head_backward(P, sv, dlogits, w2, snap=_id, norm="vl_transformer.decoder.norm.", mlp="bbox_embed.layers."):
    """sv: t3, (hstats), y1, y2 as stored (their > 0 are the gates); dlogits [R, 4]; w2: the last Linear's weight as its
    backward-data reads it (the fp32 master)."""
    r = {}
    r["dy2"] = (dlogits @ w2) * (sv["y2"] > 0)
    dy2 = snap("dy2", r["dy2"])
    r["dy1"] = (dy2 @ P[mlp + "1.weight"]) * (sv["y1"] > 0)
    dy1 = snap("dy1", r["dy1"])
    r["dhs"] = dy1 @ P[mlp + "0.weight"]
    dhs = snap("dhs", r["dhs"])
    r["dnorm"] = ln_bwd(dhs, sv["t3"], P[norm + "weight"], sv.get("hstats"))
    r["dgamma_rows"], r["dbeta_rows"] = ln_param_rows(dhs, sv["t3"], sv.get("hstats"))
    return r


# ---------------------------------------------------------------------------------------------- decoder layer
def attention(q, k, v, kpm, H, scale):
    """q [B, Tq, E], k / v [B, Tk, E], kpm [B, Tk] bool (True = ignore) or None -> o [B, Tq, E], lse [B, H, Tq], p [B, H, Tq, Tk]"""
    B, Tq, E = q.shape
    dh = E // H
    hd = lambda x: x.view(B, -1, H, dh).transpose(1, 2)        # noqa: E731
    s = (hd(q) @ hd(k).transpose(-1, -2)) * scale
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ hd(v)).transpose(1, 2).reshape(B, Tq, E), torch.logsumexp(s, dim=-1), p


def decoder_layer(P, p, t32, t16, tq16, qpos, mem16, memp16, qmask, kpm, H, snap=_id, gq=_id, hdn_gate=None, attn=None):
    """TransformerDecoderLayer.forward_post, broken at the tensors dec_layer_fwd saves.  t32: the residual stream [B, T, E];
    t16 / tq16: the stream / stream + query_pos as the projections read them; mem16 / memp16: memory / memory + pos as the
    cross-attention's K / V projections read them [B, S, E]; qmask [B, T] / kpm [B, S] bool, True = ignore.
    gq(name, y): called on the three products whose upstream gradient the backward kernels hand on as a bf16 operand although the
    forward keeps their sum with the residual in fp32 (out_proj, out_proj of the cross-attention, linear2): the identity going
    forward, a place to round the gradient coming back.  hdn_gate: the ReLU's gate as a tensor instead of the product's own sign.
    attn: stands in for `attention` (same arguments, returns (o, lse, p)), for a twin with its own attention backward."""
    att = attention if attn is None else attn
    B, T, E = t32.shape
    scale = (E // H) ** -0.5
    Wi, bi = P[p + "self_attn.in_proj_weight"], P[p + "self_attn.in_proj_bias"]
    Wc, bc = P[p + "multihead_attn.in_proj_weight"], P[p + "multihead_attn.in_proj_bias"]
    W = lambda n: (P[p + n + "weight"], P[p + n + "bias"])        # noqa: E731
    r = {}
    r["v"] = lin(t16, Wi[2 * E:], bi[2 * E:])
    if T == 1:                      # one key: the softmax is exactly 1
        r["o"] = r["v"]
    else:
        r["qk"] = lin(tq16, Wi[:2 * E], bi[:2 * E])
        qk, v = snap("qk", r["qk"]), snap("v", r["v"])
        r["o"], r["lse"], _ = att(qk[..., :E], qk[..., E:], v, qmask, H, scale)
    o = snap("o", r["o"])
    r["u"] = gq("du", lin(o, *W("self_attn.out_proj."))) + t32
    u = snap("u", r["u"])
    r["t1"] = ln(u, *W("norm1."))
    r["t1q"] = r["t1"] + qpos
    t1, t1q16 = snap("t1", r["t1"]), snap("t1q16", r["t1q"])
    r["q2"] = lin(t1q16, Wc[:E], bc[:E])
    r["k2"] = lin(memp16, Wc[E:2 * E], bc[E:2 * E])
    r["v2"] = lin(mem16, Wc[2 * E:], bc[2 * E:])
    q2, k2, v2 = snap("q2", r["q2"]), snap("k2", r["k2"]), snap("v2", r["v2"])
    r["o2"], r["lse2"], _ = att(q2, k2, v2, kpm, H, scale)
    o2 = snap("o2", r["o2"])
    r["u2"] = gq("du2", lin(o2, *W("multihead_attn.out_proj."))) + t1
    u2 = snap("u2", r["u2"])
    r["t2"] = ln(u2, *W("norm2."))
    t2, t2_16 = snap("t2", r["t2"]), snap("t2_16", r["t2"])
    h1 = lin(t2_16, *W("linear1."))
    r["hdn"] = torch.relu(h1) if hdn_gate is None else h1 * hdn_gate
    hdn = snap("hdn", r["hdn"])
    r["u3"] = gq("du3", lin(hdn, *W("linear2."))) + t2
    u3 = snap("u3", r["u3"])
    r["t3"] = ln(u3, *W("norm3."))
    r["t3q"] = r["t3"] + qpos
    return r
