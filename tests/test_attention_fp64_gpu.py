"""GPU: rt_attn_fwd / rt_attn_bwd on every dispatch path, element by element against float64 (oracle/attention_ref.py, pinned
to autograd, and its bounds proven usable and sharp on a CPU emulation of the kernels' rounding points, by
tests/test_attention_ref_cpu.py, whose cases, inputs and check functions this file runs on the kernels).

  1. dense    o, lse, dq, dk, dv of every case at the bounds derived from the number formats (no element left out; rows of masked
              keys in dk / dv exactly zero), q ~ N(0, 1) and q ~ 4 N(0, 1), without dropout and with p = 0.1; the backward is
              teacher-forced with the kernel's own o and lse
  2. probes   the probability and dS matrices read out of the kernels one (query, key) pair at a time through one-hot operands,
              the window swept over the whole axis, dropout on: a wrong key, mask bit, dropout bit or chunk offset is a whole
              element there instead of 1 / Sk of one
  3. strides  operands and results as column slices of padded packed buffers: the same bits as the contiguous run, every byte
              outside the owned rows and columns untouched; the BERT form (thirds of one [B L, 3 Hd] buffer); dh = 48 and a row
              stride that is no multiple of 8 answer RT_ERR_UNSUPPORTED and write nothing
  4. a fully masked image: its out rows are NaN and its lse -inf, and the NaN stays inside that image

Worst error / bound per kernel over its cases, both score scales and both dropout settings, measured on the MI355X (every test
prints its own).  Stored bf16 values sit just under 1: half an ulp is the rounding every one of them makes; fp32 terms (lse) use a few
per cent of their bound:
  forward   reg8      o 0.88, lse 0.01        reg28  o 0.69, lse 0.01        two-pass  o 0.65, lse 0.01
            long      o 0.74, lse 0.01        q1     o 0.89, lse 0.01
  backward  fused     dq 0.75, dk 0.91, dv 0.92        long  dq 0.83, dk 0.81, dv 0.88        q1  dq 0.86, dk 0.98, dv 0.98
  probes    A pt 0.97, B pt 0.97, C dS 0.99, D dS 0.97 (single stored bf16 values: half an ulp of each)
  BERT form o 0.66, lse 0.01, dq 0.66, dk 0.57, dv 0.55; beside a fully masked image o 0.88, lse 0.01
The masked image's lse holds -inf on both forward kernels that can meet one (reg8, q1).  The whole file (41 tests) takes 8 s on the
MI355X.

Scratch mutations of csrc/rt_attention.hip (values only, on a copy, not committed) and what noticed them:
  dkv_chunk's dropout index with Sq and Sk exchanged    dense dk at all 14 cases with Sq > 1 and probes B, D at 7; tests/test_ops_gpu.py: nothing
  c0 left out of fwd_pv_chunk's dropout index           dense o at both long-axis cases, probe A at Sk = 801; tests/test_ops_gpu.py: nothing
  attn_fwd_reg_kernel's sBias from image 0's mask       dense, probes, BERT form and the fully masked image at every B > 1 case on reg8;
                                                        tests/test_ops_gpu.py: 3 cases of test_attention_fwd_bwd
"""
import pytest
import torch

from oracle import attention_ref as A
from test_attention_ref_cpu import (ALL_CASES, P_DROP, PROBE_CASES, SCALES, SEED, check_dense, check_probes, cid, hold_backward, hold_forward,
                                    make_inputs, make_kpm, true_keep)
from test_region_fp64_gpu import Worst

pytestmark = pytest.mark.gpu

UNSUPPORTED = "code -2"                  # RT_ERR_UNSUPPORTED (include/reftr_hip.h)
PATTERN = 0x5A5B                         # the int16 pattern buffers are pre-filled with (a finite bf16, 1.5e16)


# ------------------------------------------------------------------------------------------------ the kernels behind the runner interface
class Kernels:
    """fwd / bwd as attention_ref.Emulator has them: float64 [B, S, E] tensors in, float64 results out"""

    def __init__(self, hip, case, p_drop):
        self.hip, self.case, self.p = hip, case, p_drop
        hip.set_seed_dev(None)                                # the dropout site is the plain seed

    def _kw(self):
        B, H, Sq, Sk, dh = self.case
        return dict(B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, scale=dh ** -0.5, drop_p=self.p, drop_seed=SEED)

    @staticmethod
    def dev(t):
        return t.reshape(-1, t.shape[-1]).to(torch.bfloat16).cuda().contiguous()

    @staticmethod
    def mask(kpm):
        return kpm.to(torch.uint8).cuda().contiguous()

    def host(self, t, S):
        return t.contiguous().double().cpu().view(self.case[0], S, -1)

    def fwd(self, q, k, v, kpm):
        o, lse = self.hip.attn_fwd(self.dev(q), self.dev(k), self.dev(v), self.mask(kpm), **self._kw())
        return self.host(o, self.case[2]), lse.double().cpu()

    def bwd(self, q, k, v, o, do, lse, kpm):
        dq, dk, dv = self.hip.attn_bwd(self.dev(q), self.dev(k), self.dev(v), self.dev(o), self.dev(do), lse.float().cuda().contiguous(),
                                       self.mask(kpm), **self._kw())
        return self.host(dq, self.case[2]), self.host(dk, self.case[3]), self.host(dv, self.case[3])


# ------------------------------------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
def test_dense_against_float64(hip, case):
    fwd, bwd, _ = A.dispatch(*case[2:])
    w = Worst()
    for qs in SCALES:
        x = make_inputs(case, 0, qs)
        for p_drop in (0.0, P_DROP):
            check_dense(w, Kernels(hip, case, p_drop), x, p_drop)
    print(w.line(f"dense {cid(case)} fwd {fwd} bwd {bwd}"))


# ------------------------------------------------------------------------------------------------ 2. probes
@pytest.mark.parametrize("case", PROBE_CASES, ids=cid)
def test_probability_and_ds_matrices_pair_by_pair(hip, case):
    fwd, bwd, _ = A.dispatch(*case[2:])
    w = Worst()
    for qs in SCALES:
        check_probes(w, Kernels(hip, case, P_DROP), make_inputs(case, 0, qs), P_DROP)
    print(w.line(f"probes {cid(case)} fwd {fwd} bwd {bwd}"))


# ------------------------------------------------------------------------------------------------ 3. strides and ownership
def _filled(rows, cols, dtype=torch.bfloat16):
    t = torch.empty(rows, cols, dtype=dtype, device="cuda")
    t.view(torch.int16).fill_(PATTERN)
    return t


def _place(buf, c0, src):
    """src [rows, E] into columns c0 .. c0 + E of buf; returns that view"""
    view = buf[:, c0:c0 + src.shape[1]]
    view.copy_(src)
    return view


def _untouched(buf, owned, rows=None):
    """every element of buf outside the column ranges `owned` of its first `rows` rows still holds the pattern"""
    rows = buf.shape[0] if rows is None else rows
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    for c0, c1 in owned:
        keep[c0:c1] = False
    bits = buf.view(torch.int16)
    return bool((bits[:rows][:, keep] == PATTERN).all()) and bool((bits[rows:] == PATTERN).all())


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dh", [32, 64])
def test_strided_operands_same_bits_and_nothing_else_written(hip, dh):
    """q, k, v as column slices of padded packed buffers (row strides E + 8, 2E + 16, 2E + 16), out and dout at E + 24, dq in its
    own buffer at E + 40, dk | dv as halves of one buffer at 2E + 8."""
    case = (2, 2, 37, 45, dh)
    B, H, Sq, Sk, _ = case
    E = H * dh
    x = make_inputs(case, 3)
    run = Kernels(hip, case, P_DROP)
    q, k, v, do, kpm = run.dev(x["q"]), run.dev(x["k"]), run.dev(x["v"]), run.dev(x["do"]), run.mask(x["kpm"])
    kw = run._kw()
    o0, lse0 = hip.attn_fwd(q, k, v, kpm, **kw)
    dq0, dk0, dv0 = hip.attn_bwd(q, k, v, o0, do, lse0, kpm, **kw)
    qb, kvb = _filled(B * Sq, E + 8), _filled(B * Sk, 2 * E + 16)
    ob, dob, dqb, dkvb = _filled(B * Sq + 3, E + 24), _filled(B * Sq, E + 24), _filled(B * Sq + 3, E + 40), _filled(B * Sk + 3, 2 * E + 8)      # 3 rows past the last
    qs, ks, vs = _place(qb, 8, q), _place(kvb, 8, k), _place(kvb, E + 16, v)
    dos = _place(dob, 16, do)
    ins = [t.clone() for t in (qb, kvb, dob)]
    ov = ob[:B * Sq, 8:8 + E]
    o1, lse1 = hip.attn_fwd(qs, ks, vs, kpm, out=ov, **kw)
    assert o1.data_ptr() == ov.data_ptr() and (qs.stride(0), ks.stride(0), vs.stride(0), ov.stride(0)) == (E + 8, 2 * E + 16, 2 * E + 16, E + 24)
    dq1, dk1, dv1 = hip.attn_bwd(qs, ks, vs, ov, dos, lse1, kpm, dq=dqb[:B * Sq, 24:24 + E], dk=dkvb[:B * Sk, :E], dv=dkvb[:B * Sk, E:2 * E], **kw)
    torch.cuda.synchronize()
    assert (dq1.stride(0), dk1.stride(0), dv1.stride(0)) == (E + 40, 2 * E + 8, 2 * E + 8)
    for name, a, b in (("o", o0, o1), ("lse", lse0, lse1), ("dq", dq0, dq1), ("dk", dk0, dk1), ("dv", dv0, dv1)):
        assert torch.equal(_bits(a), _bits(b)), name
    assert _untouched(ob, [(8, 8 + E)], B * Sq) and _untouched(dqb, [(24, 24 + E)], B * Sq) and _untouched(dkvb, [(0, 2 * E)], B * Sk)
    for name, buf, was in zip(("q", "kv", "dout"), (qb, kvb, dob), ins):
        assert torch.equal(_bits(buf), _bits(was)), name + ": an operand buffer was written"


@pytest.mark.parametrize("dh", [32, 64])
def test_bert_form_thirds_of_one_buffer(hip, dh):
    """q, k, v as thirds of a [B L, 3 Hd] buffer, Sq = Sk = L, and dq | dk | dv as thirds of another: held like every dense
    case, and the same bits as the contiguous run."""
    case = (2, 2, 37, 37, dh)
    B, H, L, _, _ = case
    E = H * dh
    w = Worst()
    for p_drop in (0.0, P_DROP):
        x = make_inputs(case, 4)
        run = Kernels(hip, case, p_drop)
        keep = true_keep(case, p_drop)
        qkv, dqkv = _filled(B * L, 3 * E), _filled(B * L, 3 * E)
        q, k, v = (_place(qkv, i * E, run.dev(x[n])) for i, n in enumerate("qkv"))
        kpm, kw = run.mask(x["kpm"]), run._kw()
        o, lse = hip.attn_fwd(q, k, v, kpm, **kw)
        dq, dk, dv = hip.attn_bwd(q, k, v, o, run.dev(x["do"]), lse, kpm, dq=dqkv[:, :E], dk=dqkv[:, E:2 * E], dv=dqkv[:, 2 * E:], **kw)
        o0, lse0 = run.fwd(x["q"], x["k"], x["v"], x["kpm"])
        g0 = run.bwd(x["q"], x["k"], x["v"], o0, x["do"], lse0, x["kpm"])
        oh, lh = run.host(o, L), lse.double().cpu()
        gh = [run.host(t, L) for t in (dq, dk, dv)]
        assert torch.equal(oh, o0) and torch.equal(lh, lse0) and all(torch.equal(a, b) for a, b in zip(gh, g0))
        hold_forward(w, x, keep, p_drop, oh, lh)
        hold_backward(w, x, keep, p_drop, oh, lh, *gh)
    print(w.line(f"BERT form dh {dh}"))


def test_unsupported_head_size_and_stride_write_nothing(hip):
    B, H, Sq, Sk = 2, 2, 37, 45
    kpm = Kernels.mask(make_kpm(B, Sk))

    def launch(dh, pad):
        E = H * dh
        g = torch.Generator(device="cuda").manual_seed(dh + pad)
        rn = lambda rows: torch.randn(rows, E + pad, device="cuda", generator=g).bfloat16()[:, :E]        # noqa: E731
        q, k, v, do = rn(B * Sq), rn(B * Sk), rn(B * Sk), rn(B * Sq)
        kw = dict(B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, scale=dh ** -0.5)
        outs = [_filled(B * Sq, E + pad), _filled(B * Sq, E + pad), _filled(B * Sk, E + pad), _filled(B * Sk, E + pad)]
        ov, dqv, dkv, dvv = (t[:, :E] for t in outs)
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            hip.attn_fwd(q, k, v, kpm, out=ov, **kw)
        lse = torch.zeros(B, H, Sq, device="cuda")
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            hip.attn_bwd(q, k, v, ov, do, lse, kpm, dq=dqv, dk=dkv, dv=dvv, **kw)
        torch.cuda.synchronize()
        assert all(_untouched(t, []) for t in outs)

    launch(48, 0)                   # a head size the kernels are not built for
    launch(32, 4)                   # every row stride E + 4: no multiple of 8 (the 16-byte loads would be misaligned)


# ------------------------------------------------------------------------------------------------ 4. a fully masked image
@pytest.mark.parametrize("case", [(3, 2, 19, 45, 32), (3, 2, 1, 257, 32)], ids=cid)
def test_fully_masked_image_is_nan_and_stays_inside(hip, case):
    """Image 1 all masked, forward only: its out rows are NaN (include/reftr_hip.h: "like the reference") and its lse -inf, as
    torch's logsumexp over -inf; images 0 and 2 pass the dense check unchanged."""
    B, H, Sq, Sk, dh = case
    w = Worst()
    for p_drop in (0.0, P_DROP):
        x = make_inputs(case, 5)
        x["kpm"][1] = True
        o, lse = Kernels(hip, case, p_drop).fwd(x["q"], x["k"], x["v"], x["kpm"])
        print(f"\n[fully masked {cid(case)} p={p_drop}] lse of the masked image: {sorted(set(lse[1].reshape(-1).tolist()))}")
        assert bool(torch.isnan(o[1]).all())
        assert bool((lse[1] == float("-inf")).all())
        hold_forward(w, x, true_keep(case, p_drop), p_drop, o, lse, sel=[0, 2])
    print(w.line(f"fully masked image {cid(case)}"))
