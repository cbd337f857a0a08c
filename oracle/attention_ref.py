"""float64 reference of the masked multi-head attention kernels (rt_attn_fwd / rt_attn_bwd, csrc/rt_attention.hip), the element-wise
bounds their results must keep, and a CPU emulation of the kernels' rounding points that proves those bounds usable and sharp before
anything runs on a GPU (tests/test_attention_ref_cpu.py; the kernels themselves: tests/test_attention_fp64_gpu.py).

Layout: q [B, Sq, E], k / v [B, Sk, E] (head h at columns h dh ..), kpm [B, Sk] bool (True = ignore) or None, keep [B, H, Sq, Sk] bool
(True = kept) or None, all values float64.  The dropout bit of (b, h, i, j) is the shared counter hash at index
((b H + h) Sq + i) Sk + j (keep_mask); kept probabilities are scaled by ks = the fp32 value 1 / (1 - fp32(p)).

The backward is teacher-forced: p = exp(scale q k + bias - lse_stored) and delta = dO . O_stored from the tensors the forward kernel
stored, which is what the kernels compute (row_delta and the fragment sum of attn_bwd_dq_body).

Bounds, from the number formats alone (U32 = 2^-23, U16 = 2^-8: bf16 has 7 fraction bits, so its unit roundoff is U16 itself):
  score          dh exact bf16 x bf16 products summed in fp32, times scale: ds = (dh + 3) U32 scale |q| |k|^T, zero at masked keys
  probabilities  the score bound through the softmax, dp = p (ds + sum_j p ds), + (Sk + 8) U32 p for the row sum, its reciprocal and
                 the products with it and with ks; __expf / __logf are held by the project's per-row softmax gate: an error row e
                 with ||e|| <= 1e-5 ||p row||, which reaches a sum over that row's keys as 1e-5 ||p row|| ||weights|| (Cauchy-Schwarz)
                 and a single element, or a sum over queries, as 1e-5 ||p row|| per element
  MFMA operands  the dropped, scaled probabilities pt are rounded to bf16 before P V and dV (U16 pt), dS before dQ and dK (U16 |dS|);
                 the Sq = 1 kernels (attn_q1_*_kernel) keep both in fp32: mfma=False drops the two terms
  sums           n terms accumulated in fp32: (n + 2) U32 sum |terms|
  dS             cancels (dP - delta): its fp32 error is measured against the pieces, p scale (dh + 3) U32 (keep ks |dO| |V|^T +
                 |dO| . |O_stored|), plus the relative error of p (ds + 4 U32, and the exp gate)
  bf16 stores    U16 (|ref| + stage bound)
  lse            max_j ds + 1e-5 |lse|
A masked or dropped element has a zero bound: it must be exact.
Test infrastructure: nothing under reftr_amd/ imports this module.
"""
import numpy as np
import torch

from . import region_ref as R

U32, U16 = 2.0 ** -23, 2.0 ** -8
GATE = 1e-5                       # the per-row softmax gate of tests/test_ops_gpu.py (what __expf / __logf may cost)
Q1_MAXK = 3 * 256                 # the longest key axis of the Sq = 1 kernels


# ---------------------------------------------------------------------------------------------- layout, dispatch, dropout bits
def heads(x, H):
    B, S, E = x.shape
    return x.view(B, S, H, E // H).transpose(1, 2)


def merge(x):
    B, H, S, dh = x.shape
    return x.transpose(1, 2).reshape(B, S, H * dh)


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def lds_bytes(inner, dh):
    ip = (inner + 31) & ~31
    return 2 * ip * (dh * 2 + 32) + 8 * ip


def long_chunk(inner, dh):
    """rows per LDS pass of the long-axis kernels, 0 where the whole axis fits the CU's 160 KB"""
    return (768 if dh == 32 else 448) if lds_bytes(inner, dh) > 160 * 1024 else 0


def dispatch(Sq, Sk, dh):
    """(forward kernel, backward kernel, chunk of the backward) rt_attn_fwd / rt_attn_bwd choose for a shape"""
    if Sq == 1 and dh == 32 and Sk <= Q1_MAXK:
        return "q1", "q1", 0
    tiles = ((Sk + 31) & ~31) >> 4
    fwd = "long" if long_chunk(Sk, dh) else "reg8" if tiles <= 8 else "reg28" if tiles <= 28 else "two-pass"
    ch = max(long_chunk(Sk, dh), long_chunk(Sq, dh))
    return fwd, "long" if ch else "fused", ch


def keep_mask(hash_keep, seed, p, B, H, Sq, Sk, swap=False, chunk_k=0, chunk_q=0):
    """keep bits [B, H, Sq, Sk] of the index ((b H + h) Sq + i) Sk + j (uint32 arithmetic, as the kernels').  The wrong forms a
    kernel could compute instead: swap = Sq and Sk exchanged; chunk_k / chunk_q = the index within its chunk, the chunk's offset
    left out."""
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    i = np.arange(Sq, dtype=np.uint64).reshape(1, 1, Sq, 1)
    j = np.arange(Sk, dtype=np.uint64).reshape(1, 1, 1, Sk)
    if chunk_q:
        i = i % np.uint64(chunk_q)
    if chunk_k:
        j = j % np.uint64(chunk_k)
    a, b = (Sk, Sq) if swap else (Sq, Sk)
    idx = ((bh * np.uint64(a) + i) * np.uint64(b) + j) & np.uint64(0xFFFFFFFF)
    return torch.from_numpy(hash_keep(seed, idx.reshape(-1), p).reshape(B, H, Sq, Sk))


def _mult(keep, p_drop, like):
    return torch.ones_like(like) if keep is None else keep.to(like.dtype) * drop_scale(p_drop)


def _valid(kpm, like):
    return torch.ones_like(like) if kpm is None else (~kpm)[:, None, None, :].to(like.dtype).expand_as(like)


# ---------------------------------------------------------------------------------------------- the reference
def forward(q, k, v, kpm, keep, p_drop, H, scale):
    """-> o [B, Sq, E], lse [B, H, Sq], p [B, H, Sq, Sk], pt = p keep ks"""
    _, lse, p = R.attention(q, k, v, kpm, H, scale)
    pt = p * _mult(keep, p_drop, p)
    return merge(pt @ heads(v, H)), lse, p, pt


def backward(q, k, v, o_stored, do, lse_stored, kpm, keep, p_drop, H, scale):
    """-> dict(dq, dk, dv [B, S, E]; dS, pt, p, c = (dP - delta) scale [B, H, Sq, Sk]; delta [B, H, Sq])"""
    qh, kh, vh, oh, doh = (heads(x, H) for x in (q, k, v, o_stored, do))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    p = torch.exp(s - lse_stored[..., None])
    m = _mult(keep, p_drop, p)
    delta = (doh * oh).sum(-1)
    c = (m * (doh @ vh.transpose(-1, -2)) - delta[..., None]) * scale
    dS, pt = p * c, p * m
    return dict(dq=merge(dS @ kh), dk=merge(dS.transpose(-1, -2) @ qh), dv=merge(pt.transpose(-1, -2) @ doh), dS=dS, pt=pt, p=p, c=c,
                delta=delta)


# ---------------------------------------------------------------------------------------------- bounds
def score_bound(q, k, kpm, H, scale):
    dh = q.shape[-1] // H
    ds = (dh + 3) * U32 * scale * (heads(q.abs(), H) @ heads(k.abs(), H).transpose(-1, -2))
    return ds if kpm is None else ds.masked_fill(kpm[:, None, None, :], 0.0)


def stored(ref, stage):
    """a bf16 store of a value whose fp32 form is within `stage` of ref"""
    return stage + U16 * (ref.abs() + stage)


def forward_bounds(q, k, v, kpm, keep, p_drop, H, scale, o, lse, p, pt, mfma=True):
    """-> dict(o, lse, pt): pt = the bound of one probability read out through a one-hot V (probe A)"""
    Sk = k.shape[1]
    ds = score_bound(q, k, kpm, H, scale)
    m = _mult(keep, p_drop, p)
    dp = p * (ds + (p * ds).sum(-1, keepdim=True)) + (Sk + 8) * U32 * p
    g = GATE * p.norm(dim=-1, keepdim=True)
    va = heads(v.abs(), H)
    ptv = pt @ va
    stage = (dp * m) @ va + g * ((m * m) @ (va * va)).sqrt() + (Sk + 2) * U32 * ptv + (U16 * ptv if mfma else 0.0)
    live = m * (p > 0)                                       # a masked or dropped probability is exactly zero
    return dict(o=stored(o, merge(stage)), lse=ds.amax(-1) + GATE * lse.abs(), pt=stored(pt, (dp + g) * live))


def backward_bounds(q, k, v, o_stored, do, kpm, keep, p_drop, H, scale, b, mfma=True):
    """b: backward()'s result.  -> dict(dq, dk, dv; dS, pt = the bounds of one element read out by the probes B, C, D)"""
    dh, Sq, Sk = q.shape[-1] // H, q.shape[1], k.shape[1]
    p, pt, dS, c = b["p"], b["pt"], b["dS"], b["c"]
    m = _mult(keep, p_drop, p)
    live = (p > 0).to(p.dtype)
    rp = score_bound(q, k, kpm, H, scale) + 4 * U32          # p = exp(s - lse_stored): no row sum here
    g = GATE * p.norm(dim=-1, keepdim=True)
    qa, ka, va, oa, doa = (heads(x.abs(), H) for x in (q, k, v, o_stored, do))
    pieces = m * (doa @ va.transpose(-1, -2)) + (doa * oa).sum(-1, keepdim=True)
    e_ds = p * scale * (dh + 3) * U32 * pieces + rp * dS.abs()          # fp32 dS, without the exp gate
    g_ds = g * c.abs() * live
    e_pt = rp * pt + g * m * live
    r16 = U16 if mfma else 0.0
    op_ds = e_ds + r16 * dS.abs()                            # the operand of dQ and dK
    dq = op_ds @ ka + ((g_ds * g_ds) @ (ka * ka)).sqrt() + (Sk + 2) * U32 * (dS.abs() @ ka)
    dk = (op_ds + g_ds).transpose(-1, -2) @ qa + (Sq + 2) * U32 * (dS.abs().transpose(-1, -2) @ qa)
    dv = (e_pt + r16 * pt).transpose(-1, -2) @ doa + (Sq + 2) * U32 * (pt.transpose(-1, -2) @ doa)
    return dict(dq=stored(b["dq"], merge(dq)), dk=stored(b["dk"], merge(dk)), dv=stored(b["dv"], merge(dv)),
                dS=stored(dS, e_ds + g_ds), pt=stored(pt, e_pt))


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic on the CPU
MUTANTS = ("tail_short", "keep_bit", "dkv_swap", "no_c0", "pad_tile", "kpm_image0", "delta_unrounded")


class Emulator:
    """rt_attn_fwd / rt_attn_bwd in torch fp32 on the CPU: fp32 scores and softmax, .bfloat16() at exactly the rounding points listed
    above (none inside the Sq = 1 kernels), fp32 products, bf16 stores.  `mutant` switches one wrong kernel on:
      tail_short       (a) the masked tail one key short: its first key is read as valid
      keep_bit         (b) one key's keep bit inverted (key Sk // 2 of every row)
      dkv_swap         (c) the dK / dV half's dropout index built with Sk and Sq exchanged
      no_c0            (d) the chunk's offset left out of the dropout index beyond the first chunk (keys in the forward and the dQ
                           half, queries in the dK / dV half)
      pad_tile         (e) the last 16-key tile of a padded row not masked: its zero keys take part in the softmax
      kpm_image0       (f) the key-padding mask read with image 0's row for every image
      delta_unrounded  (g) delta from the forward's fp32 output instead of the stored bf16 one
    fwd / bwd take and return float64 tensors (bf16-representable inputs), like the GPU runner of the kernel tests."""

    def __init__(self, H, scale, hash_keep=None, p_drop=0.0, seed=0, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.H, self.scale, self.hash_keep, self.p, self.seed, self.mutant = H, scale, hash_keep, p_drop, seed, mutant
        self.o32 = None

    def _keep(self, B, Sq, Sk, dh, half):
        if not self.p > 0:
            return None
        kw = {}
        if self.mutant == "dkv_swap" and half == "dkv":
            kw["swap"] = True
        if self.mutant == "no_c0":
            fwd, bwd, ch = dispatch(Sq, Sk, dh)
            if half == "fwd" and fwd == "long":
                kw["chunk_k"] = long_chunk(Sk, dh)
            if half == "dq" and bwd == "long":
                kw["chunk_k"] = ch
            if half == "dkv" and bwd == "long":
                kw["chunk_q"] = ch
        keep = keep_mask(self.hash_keep, self.seed, self.p, B, self.H, Sq, Sk, **kw)
        if self.mutant == "keep_bit":
            keep = keep.clone()
            keep[..., Sk // 2] = ~keep[..., Sk // 2]
        return keep

    def _kpm(self, kpm):
        if kpm is None:
            return None
        if self.mutant == "kpm_image0":
            return kpm[:1].expand_as(kpm)
        if self.mutant == "tail_short":
            kpm = kpm.clone()
            for b in range(kpm.shape[0]):
                t = kpm.shape[1]
                while t > 0 and kpm[b, t - 1]:
                    t -= 1
                if t < kpm.shape[1]:
                    kpm[b, t] = False
        return kpm

    def _scores(self, q, k, kpm):
        s = (heads(q.float(), self.H) @ heads(k.float(), self.H).transpose(-1, -2)) * np.float32(self.scale)
        kpm = self._kpm(kpm)
        return s if kpm is None else s.masked_fill(kpm[:, None, None, :], float("-inf"))

    def fwd(self, q, k, v, kpm):
        B, Sq, E = q.shape
        Sk, dh = k.shape[1], E // self.H
        mfma = dispatch(Sq, Sk, dh)[0] != "q1"
        s = self._scores(q, k, kpm)
        if self.mutant == "pad_tile" and mfma:
            Skp = (Sk + 31) & ~31
            extra = Skp - max(Sk, Skp - 16)                 # keys of the last tile past Sk: zero K rows, score 0
            s = torch.cat([s, s.new_zeros(B, self.H, Sq, extra)], dim=-1)
        mx = s.amax(-1, keepdim=True)
        ms = torch.where(mx == float("-inf"), torch.zeros_like(mx), mx)
        e = torch.exp(s - ms)
        l = e.sum(-1, keepdim=True)
        pr = (e * (1.0 / l))[..., :Sk]
        keep = self._keep(B, Sq, Sk, dh, "fwd")
        if keep is not None:
            pr = torch.where(keep, pr * np.float32(drop_scale(self.p)), torch.zeros_like(pr))
        if mfma:
            pr = pr.bfloat16().float()
        self.o32 = merge(pr @ heads(v.float(), self.H))
        return self.o32.bfloat16().double(), (mx + torch.log(l)).squeeze(-1).double()

    def bwd(self, q, k, v, o, do, lse, kpm):
        B, Sq, E = q.shape
        Sk, dh, H = k.shape[1], E // self.H, self.H
        mfma = dispatch(Sq, Sk, dh)[1] != "q1"
        qh, kh, vh, doh = (heads(x.float(), H) for x in (q, k, v, do))
        oh = heads(self.o32 if self.mutant == "delta_unrounded" else o.float(), H)
        pr = torch.exp(self._scores(q, k, kpm) - lse.float()[..., None])
        dp = doh @ vh.transpose(-1, -2)
        delta = (doh * oh).sum(-1, keepdim=True)
        ks = np.float32(drop_scale(self.p))
        res = {}
        for half in ("dq", "dkv"):
            keep = self._keep(B, Sq, Sk, dh, half)
            d, pd = dp, pr
            if keep is not None:
                d = torch.where(keep, dp * ks, torch.zeros_like(dp))
                pd = torch.where(keep, pr * ks, torch.zeros_like(pr))
            ds = pr * (d - delta) * np.float32(self.scale)
            if mfma:
                ds, pd = ds.bfloat16().float(), pd.bfloat16().float()
            if half == "dq":
                res["dq"] = merge(ds @ kh)
            else:
                res["dk"], res["dv"] = merge(ds.transpose(-1, -2) @ qh), merge(pd.transpose(-1, -2) @ doh)
        return tuple(res[n].bfloat16().double() for n in ("dq", "dk", "dv"))
