"""CPU: oracle/attention_ref.py, the float64 reference and the element-wise bounds tests/test_attention_fp64_gpu.py holds
rt_attn_fwd / rt_attn_bwd to.

  1. forward / backward against float64 autograd through plain softmax(masked_fill) . keep . ks @ v with the exact o and lse fed
     back: outputs and the three gradients to 1e-12 relative at every GPU case shape
  2. the bounds hold for a CPU emulation of the kernels' rounding points (attention_ref.Emulator) at every GPU case, 5 seeds, both
     score scales, dropout off and on: every error / bound <= 1, no element left out, through the same check functions the GPU
     file runs on the kernels (the cases, inputs and checks below are the GPU file's too)
  3. each wrong kernel the emulator can switch on exceeds a bound, in the check and at the case named in MUTANT_TESTS

Worst error / bound of the clean emulator over all cases, seeds and scales:
  dense   o 0.92, lse 0.01, dq 0.90, dk 0.98, dv 0.98 (dk, dv: the Sq = 1 kernels, one bf16 store of one product)
  probes  A pt 0.97, B pt 0.97, C dS 0.99, D dS 0.97
"""
import math

import numpy as np
import pytest
import torch

from oracle import attention_ref as A
from test_gemm_gpu import hash_keep
from test_region_fp64_gpu import Worst, hold

P_DROP, SEED = 0.1, 4242

# (B, H, Sq, Sk, dh) per dispatch path: the smallest shape that reaches it, B >= 2 and H >= 2 wherever the index arithmetic holds them
CASES = {
    "reg8 dh32": [(2, 2, 37, 45, 32)],                       # ragged third wave, waves 3-7 return early, Skp = 64 with 19 padded keys
    "reg8 dh64": [(2, 2, 37, 45, 64)],
    "second row block": [(1, 2, 130, 45, 32)],               # blockIdx.y = 1 with two live rows
    "reg28": [(1, 2, 19, 130, 32), (1, 2, 19, 130, 64), (1, 1, 16, 448, 32)],          # 10 of 28 tiles, then all 28
    "two-pass": [(1, 2, 19, 449, 32), (1, 1, 17, 800, 32), (1, 2, 19, 470, 64), (1, 1, 16, 480, 64)],   # up to the last one-pass length
    "long axis": [(1, 2, 19, 801, 32), (1, 2, 19, 481, 64)],                            # chunks 768 + 64 and 448 + 64
    "long in the backward only": [(1, 1, 801, 33, 32), (1, 1, 481, 19, 64)],            # forward on reg8, backward long through Sq
    "Sq = 1 kernels": [(3, 2, 1, Sk, 32) for Sk in (1, 255, 256, 257, 512, 513, 768)],  # 1, 2 and 3 keys per thread and their edges
    "Sq = 1 on the MFMA kernels": [(2, 2, 1, 769, 32), (2, 2, 1, 45, 64)],
}
PATHS = {"reg8 dh32": ("reg8", "fused"), "reg8 dh64": ("reg8", "fused"), "second row block": ("reg8", "fused"), "reg28": ("reg28", "fused"),
         "two-pass": ("two-pass", "fused"), "long axis": ("long", "long"), "long in the backward only": ("reg8", "long"),
         "Sq = 1 kernels": ("q1", "q1")}
ALL_CASES = [c for row in CASES.values() for c in row]
PROBE_CASES = [row[0] for name, row in CASES.items() if name != "Sq = 1 kernels"] + [(3, 2, 1, Sk, 32) for Sk in (1, 257, 768)]
SCALES = (1.0, 4.0)                     # q ~ N(0, 1) and the peaked scores of q ~ 4 N(0, 1)


def cid(c):
    return "x".join(str(n) for n in c)


# ------------------------------------------------------------------------------------------------ inputs
def make_kpm(B, Sk):
    """A key-padding mask that differs per image: key 0 and the tile edges 15 | 16 and 31 | 32 where they exist, and a masked tail
    of (b + 1) max(2, Sk // 40) keys (short enough to leave valid keys in the last chunk of a long axis) -- but in the last of
    several images only the last key.  Never a fully masked row (Sk = 1: no bit)."""
    kpm = torch.zeros(B, Sk, dtype=torch.bool)
    if Sk == 1:
        return kpm
    for b in range(B):
        tail = 1 if (B > 1 and b == B - 1) else (b + 1) * max(2, Sk // 40)
        kpm[b, Sk - tail:] = True
    for j in (0, 15, 16, 31, 32):
        if j < Sk:
            kpm[:, j] = True
    assert bool((~kpm).any(1).all())
    return kpm


def make_inputs(case, seed=0, qscale=1.0):
    B, H, Sq, Sk, dh = case
    E = H * dh
    g = torch.Generator().manual_seed(1000 * seed + Sq + Sk + dh)
    bf = lambda t: t.bfloat16().double()        # noqa: E731
    return dict(case=case, H=H, scale=dh ** -0.5, q=bf(qscale * torch.randn(B, Sq, E, generator=g)), k=bf(torch.randn(B, Sk, E, generator=g)),
                v=bf(torch.randn(B, Sk, E, generator=g)), do=bf(1e-2 * torch.randn(B, Sq, E, generator=g)), kpm=make_kpm(B, Sk))


def true_keep(case, p_drop, seed=SEED):
    B, H, Sq, Sk, dh = case
    if not p_drop > 0:
        return None
    keep = A.keep_mask(hash_keep, seed, p_drop, B, H, Sq, Sk)
    # 2 % - 25 % dropped at p = 0.1, as _check_qenc_fwd asserts (the six bits of the one-key case say nothing about a rate)
    assert 0.02 < float((~keep).double().mean()) < 0.25 or keep.numel() < 64
    return keep


def emulator(case, p_drop, mutant=None):
    return A.Emulator(case[1], case[4] ** -0.5, hash_keep, p_drop, SEED, mutant)


# ------------------------------------------------------------------------------------------------ checks (shared with the GPU file)
def hold_forward(w, x, keep, p_drop, o, lse, sel=None):
    """o and lse of one launch, element by element; sel: the images to check (the others hold a fully masked row)"""
    B, H, Sq, Sk, dh = x["case"]
    s = slice(None) if sel is None else sel
    q, k, v, kpm, kp = x["q"][s], x["k"][s], x["v"][s], x["kpm"][s], None if keep is None else keep[s]
    mfma = A.dispatch(Sq, Sk, dh)[0] != "q1"
    ro, rl, p, pt = A.forward(q, k, v, kpm, kp, p_drop, H, x["scale"])
    fb = A.forward_bounds(q, k, v, kpm, kp, p_drop, H, x["scale"], ro, rl, p, pt, mfma)
    hold(w, "o", o[s], ro, fb["o"])
    hold(w, "lse", lse[s], rl, fb["lse"])


def hold_backward(w, x, keep, p_drop, o, lse, dq, dk, dv):
    B, H, Sq, Sk, dh = x["case"]
    mfma = A.dispatch(Sq, Sk, dh)[1] != "q1"
    b = A.backward(x["q"], x["k"], x["v"], o, x["do"], lse, x["kpm"], keep, p_drop, H, x["scale"])
    bb = A.backward_bounds(x["q"], x["k"], x["v"], o, x["do"], x["kpm"], keep, p_drop, H, x["scale"], b, mfma)
    hold(w, "dq", dq, b["dq"], bb["dq"])
    hold(w, "dk", dk, b["dk"], bb["dk"])
    hold(w, "dv", dv, b["dv"], bb["dv"])
    for n, t in (("dk", dk), ("dv", dv)):          # masked keys: exact zeros on every path
        assert float(t[x["kpm"]].abs().sum()) == 0.0, n + ": a masked key's row is not zero"


def check_dense(w, run, x, p_drop):
    keep = true_keep(x["case"], p_drop)
    o, lse = run.fwd(x["q"], x["k"], x["v"], x["kpm"])
    hold_forward(w, x, keep, p_drop, o, lse)
    dq, dk, dv = run.bwd(x["q"], x["k"], x["v"], o, x["do"], lse, x["kpm"])
    hold_backward(w, x, keep, p_drop, o, lse, dq, dk, dv)


def _windows(n, dh):
    return range(0, n, dh)


def _onehot(B, S, H, dh, r0, value=1.0):
    """[B, S, H dh]: row r0 + d holds `value` at column h dh + d of every head, d < dh; zero elsewhere"""
    t = torch.zeros(B, S, H, dh, dtype=torch.float64)
    n = min(dh, S - r0)
    t[:, r0 + torch.arange(n), :, torch.arange(n)] = value
    return t.view(B, S, H * dh)


def _cols(t, H):
    """[B, S, H dh] -> [B, H, S, dh]"""
    return A.heads(t, H)


def check_probes(w, run, x, p_drop, which="ABCD"):
    """Read the probability and dS matrices out of the kernels one (query, key) pair at a time: with a one-hot operand a product
    over the head dimension passes single elements of pt / dS through, so a wrong key, mask bit, dropout bit or chunk offset is a
    whole element instead of 1 / Sk of one.  The window of dh pairs sweeps the whole axis."""
    B, H, Sq, Sk, dh = x["case"]
    sc, kpm = x["scale"], x["kpm"]
    keep = true_keep(x["case"], p_drop)
    fwd_mfma, bwd_mfma = (A.dispatch(Sq, Sk, dh)[i] != "q1" for i in (0, 1))
    if "A" in which:          # forward pt: V one-hot inside a window of keys -> out[i, h dh + d] = bf16(pt[i, j0 + d])
        ro, rl, p, pt = A.forward(x["q"], x["k"], x["v"], kpm, keep, p_drop, H, sc)
        fb = A.forward_bounds(x["q"], x["k"], x["v"], kpm, keep, p_drop, H, sc, ro, rl, p, pt, fwd_mfma)
        for j0 in _windows(Sk, dh):
            n = min(dh, Sk - j0)
            o, _ = run.fwd(x["q"], x["k"], _onehot(B, Sk, H, dh, j0), kpm)
            got, ref = _cols(o, H)[..., :n], pt[..., j0:j0 + n]
            hold(w, "A pt", got, ref, fb["pt"][..., j0:j0 + n])
            assert bool((got[ref > 1e-30] > 0).all()), "A pt: a kept key with weight reads zero"
    if "B" in which:          # the dK / dV half's pt: dO one-hot over a window of queries -> dv[j, h dh + d] = bf16(pt[i0 + d, j])
        o, lse = run.fwd(x["q"], x["k"], x["v"], kpm)
        for i0 in _windows(Sq, dh):
            n = min(dh, Sq - i0)
            do = _onehot(B, Sq, H, dh, i0)
            _, _, dv = run.bwd(x["q"], x["k"], x["v"], o, do, lse, kpm)
            b = A.backward(x["q"], x["k"], x["v"], o, do, lse, kpm, keep, p_drop, H, sc)
            bb = A.backward_bounds(x["q"], x["k"], x["v"], o, do, kpm, keep, p_drop, H, sc, b, bwd_mfma)
            got, ref = _cols(dv, H)[..., :n].transpose(-1, -2), b["pt"][..., i0:i0 + n, :]
            hold(w, "B pt", got, ref, bb["pt"][..., i0:i0 + n, :])
            assert bool((got[ref > 1e-30] > 0).all()), "B pt: a kept key with weight reads zero"
    if "C" in which:          # the dQ half's dS: K = c e_(j - j0) inside the window (c = 2, exact) -> dq[i, h dh + d] = c bf16(dS[i, j0 + d])
        for j0 in _windows(Sk, dh):
            n = min(dh, Sk - j0)
            k = _onehot(B, Sk, H, dh, j0, 2.0)
            o, lse = run.fwd(x["q"], k, x["v"], kpm)
            dq, _, _ = run.bwd(x["q"], k, x["v"], o, x["do"], lse, kpm)
            b = A.backward(x["q"], k, x["v"], o, x["do"], lse, kpm, keep, p_drop, H, sc)
            bb = A.backward_bounds(x["q"], k, x["v"], o, x["do"], kpm, keep, p_drop, H, sc, b, bwd_mfma)
            hold(w, "C dS", _cols(dq, H)[..., :n], 2.0 * b["dS"][..., j0:j0 + n], 2.0 * bb["dS"][..., j0:j0 + n])
    if "D" in which:          # the dK / dV half's dS: Q one-hot over a window of queries -> dk[j, h dh + d] = bf16(dS[i0 + d, j])
        for i0 in _windows(Sq, dh):
            n = min(dh, Sq - i0)
            q = _onehot(B, Sq, H, dh, i0)
            o, lse = run.fwd(q, x["k"], x["v"], kpm)
            _, dk, _ = run.bwd(q, x["k"], x["v"], o, x["do"], lse, kpm)
            b = A.backward(q, x["k"], x["v"], o, x["do"], lse, kpm, keep, p_drop, H, sc)
            bb = A.backward_bounds(q, x["k"], x["v"], o, x["do"], kpm, keep, p_drop, H, sc, b, bwd_mfma)
            hold(w, "D dS", _cols(dk, H)[..., :n].transpose(-1, -2), b["dS"][..., i0:i0 + n, :], bb["dS"][..., i0:i0 + n, :])


# ------------------------------------------------------------------------------------------------ 0. the cases reach their kernels
def test_cases_reach_the_kernels_they_name():
    for name, row in CASES.items():
        for (B, H, Sq, Sk, dh) in row:
            fwd, bwd, ch = A.dispatch(Sq, Sk, dh)
            if name == "Sq = 1 on the MFMA kernels":
                assert fwd != "q1" and bwd != "q1" and Sq == 1
            else:
                assert (fwd, bwd) == PATHS[name], (name, Sq, Sk, dh, fwd, bwd)
    # the thresholds themselves: one key less stays on the shorter path
    assert A.dispatch(19, 448, 64)[0] == "reg28" and A.dispatch(19, 449, 64)[0] == "two-pass"
    assert A.dispatch(19, 800, 32)[0] == "two-pass" and A.dispatch(19, 480, 64)[0] == "two-pass"
    assert A.dispatch(800, 33, 32)[1] == "fused" and A.dispatch(480, 19, 64)[1] == "fused"
    assert A.dispatch(19, 801, 32)[2] == 768 and A.dispatch(481, 19, 64)[2] == 448


# ------------------------------------------------------------------------------------------------ 1. the reference against autograd
def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
@pytest.mark.parametrize("p_drop", [0.0, P_DROP])
def test_reference_against_autograd(case, p_drop):
    B, H, Sq, Sk, dh = case
    x = make_inputs(case, seed=1)
    keep = true_keep(case, p_drop)
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    hd = lambda t, S: t.view(B, S, H, dh).transpose(1, 2)        # noqa: E731
    s = (hd(q, Sq) @ hd(k, Sk).transpose(-1, -2)) * x["scale"]
    s = s.masked_fill(x["kpm"][:, None, None, :], float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep * A.drop_scale(p_drop)
    out = (pr @ hd(v, Sk)).transpose(1, 2).reshape(B, Sq, H * dh)
    out.backward(x["do"])
    o, lse, p, pt = A.forward(x["q"], x["k"], x["v"], x["kpm"], keep, p_drop, H, x["scale"])
    assert rel(o, out.detach()) < 1e-12 and rel(lse, torch.logsumexp(s.detach(), -1)) < 1e-12 and rel(pt, pr.detach()) < 1e-12
    b = A.backward(x["q"], x["k"], x["v"], o, x["do"], lse, x["kpm"], keep, p_drop, H, x["scale"])
    assert rel(b["dq"], q.grad) < 1e-12 and rel(b["dk"], k.grad) < 1e-12 and rel(b["dv"], v.grad) < 1e-12
    assert rel(b["pt"], pt) < 1e-12
    assert float(b["dk"][x["kpm"]].abs().sum()) == 0.0 and float(b["dv"][x["kpm"]].abs().sum()) == 0.0


def test_drop_scale_is_the_fp32_value():
    assert A.drop_scale(0.1) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))) != 1.0 / 0.9
    assert A.drop_scale(0.0) == 1.0


# ------------------------------------------------------------------------------------------------ 2. the bounds hold for the emulator
@pytest.mark.parametrize("case", ALL_CASES, ids=cid)
def test_bounds_hold_for_the_clean_emulator(case):
    w = Worst()
    for seed in range(5):
        for qs in SCALES:
            x = make_inputs(case, seed, qs)
            for p_drop in (0.0, P_DROP):
                check_dense(w, emulator(case, p_drop), x, p_drop)
    print(w.line("emulator dense " + cid(case)))
    assert all(math.isfinite(v) for v in w.values())


@pytest.mark.parametrize("case", PROBE_CASES, ids=cid)
def test_probe_bounds_hold_for_the_clean_emulator(case):
    w = Worst()
    for seed in range(2):
        for qs in SCALES:
            check_probes(w, emulator(case, P_DROP), make_inputs(case, seed, qs), P_DROP)
    print(w.line("emulator probes " + cid(case)))


# ------------------------------------------------------------------------------------------------ 3. the mutants must fail
# (mutant, check, case, score scales, the outputs one of which must exceed its bound).  The dense check alone has to catch (c), (d)
# and (g); the others are caught by the dense check at q ~ N(0, 1) and by the probes at peaked scores, where a single key of a long
# row can hide inside the bf16 rounding of the probabilities.
MUTANT_TESTS = [
    ("tail_short", "dense", (2, 2, 37, 45, 32), (1.0,), "o|lse"),
    ("tail_short", "probes", (1, 2, 19, 801, 32), (4.0,), "A pt|B pt|C dS|D dS"),
    ("keep_bit", "dense", (2, 2, 37, 45, 32), (1.0,), "o"),
    ("keep_bit", "probes", (1, 2, 19, 801, 32), (4.0,), "A pt|B pt|C dS|D dS"),
    ("dkv_swap", "dense", (2, 2, 37, 45, 32), SCALES, "dk|dv"),                 # the forward and dq are right: only dk / dv can see it
    ("no_c0", "dense", (1, 2, 19, 801, 32), SCALES, "o"),
    ("no_c0", "dense", (1, 1, 801, 33, 32), SCALES, "dk|dv"),                   # long through Sq: only the dK / dV half walks chunks
    ("pad_tile", "dense", (2, 2, 37, 45, 32), SCALES, "o|lse"),
    ("pad_tile", "probes", (2, 2, 37, 45, 32), SCALES, "A pt"),
    ("kpm_image0", "dense", (2, 2, 37, 45, 32), SCALES, "o|lse"),
    ("kpm_image0", "probes", (2, 2, 37, 45, 32), SCALES, "A pt|B pt|C dS|D dS"),
    ("delta_unrounded", "dense", (3, 2, 1, 1, 32), SCALES, "dq"),               # one key: dS = p (dP - delta) cancels to rounding
    ("delta_unrounded", "dense", (2, 2, 37, 45, 32), (4.0,), "dq|dk"),
]


@pytest.mark.parametrize("mutant,check,case,scales,outputs", MUTANT_TESTS, ids=[f"{m[0]}-{m[1]}-{cid(m[2])}" for m in MUTANT_TESTS])
def test_mutants_exceed_a_bound(mutant, check, case, scales, outputs):
    assert case in (ALL_CASES if check == "dense" else PROBE_CASES)
    for seed in range(2):
        for qs in scales:
            x = make_inputs(case, seed, qs)
            w = Worst()
            with pytest.raises(AssertionError, match=rf"^({outputs}): "):
                (check_dense if check == "dense" else check_probes)(w, emulator(case, P_DROP, mutant), x, P_DROP)
            assert max(w.values()) > 1.0
