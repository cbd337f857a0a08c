"""CPU: oracle/region_ref.py (the float64 stage functions tests/test_region_fp64_gpu.py holds the kernels to) against the pinned
oracle.  The stages are composed free-running -- each feeds the next, nothing is rounded -- on random float64 inputs and the
small model's weights, and must reproduce O.query_encoder, O.decoder_layer x 2 + O.layer_norm, the head's three O.linear and
O.criterion: outputs, and autograd gradients with respect to memory, the phrase feature and every parameter of the region, to
1e-10 relative per tensor.  The hand-written backward stages (query encoder, head) must agree with autograd of the forward
stages at the same 1e-10."""
import pytest
import torch

from oracle import region_ref as R
from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.weights import formula_state

TOL = 1e-10
VT = "vl_transformer."
REGION = ("query_encoder.", VT + "decoder.", "bbox_embed.")


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.fixture(scope="module")
def small():
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2))
    P32 = formula_state(param_shapes(ocfg))
    g = torch.Generator().manual_seed(7)
    P = {k: v.double() for k, v in P32.items() if k.startswith(REGION)}
    # formula_state promises no particular value for the last Linear: give it one the gradients can flow through
    P["bbox_embed.layers.2.weight"] = 0.05 * torch.randn(P["bbox_embed.layers.2.weight"].shape, generator=g, dtype=torch.float64)
    return ocfg, P


def _inputs(B, L, HW, Pn, nq, seed, pad_phrase):
    g = torch.Generator().manual_seed(seed)
    E, S = 256, L + HW
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    d = dict(memory=rn(S, B, E), pos=rn(S, B, E), phrase=0.5 * rn(B, Pn, E))
    ctx = torch.rand(B, Pn, L, generator=g) < 0.4
    ctx[:, :, 0] = False
    d["ctx"] = ctx
    kpm = torch.rand(B, S, generator=g) < 0.2
    kpm[:, 0] = False
    d["kpm"] = kpm
    qm = torch.zeros(B, Pn, dtype=torch.bool)
    if pad_phrase:
        qm[1, Pn - 1] = True
    d["qmask"] = qm
    d["targets"] = [{"boxes": 0.3 + 0.4 * torch.rand(int((~qm[b]).sum()), 4, generator=g, dtype=torch.float64),
                     "labels": torch.zeros(int((~qm[b]).sum()), dtype=torch.long)} for b in range(B)]
    return d


def _oracle_forward(P, d, ocfg, nq):
    L = d["ctx"].shape[-1]
    B, Pn = d["qmask"].shape
    tgt, qpos = O.query_encoder(P, d["memory"][:L].transpose(0, 1), d["phrase"], d["ctx"], ocfg)
    qmask = d["qmask"][:, :, None].expand(-1, -1, nq).reshape(B, Pn * nq)
    t, ts, hs = tgt, [], []
    for i in range(ocfg.dec_layers):
        t = O.decoder_layer(t, d["memory"], qpos, d["pos"], qmask, d["kpm"], P, f"{VT}decoder.layers.{i}.", ocfg)
        ts.append(t)
        hs.append(O.layer_norm(t, P, VT + "decoder.norm."))
    h = torch.stack(hs).transpose(1, 2).reshape(len(hs), B, Pn, nq, -1)
    y = torch.relu(O.linear(h, P, "bbox_embed.layers.0."))
    y = torch.relu(O.linear(y, P, "bbox_embed.layers.1."))
    logits = O.linear(y, P, "bbox_embed.layers.2.")
    return dict(tgt=tgt, qpos=qpos, ts=ts, hs=h, logits=logits, valid=~qmask)


def _stage_forward(P, d, ocfg, nq):
    L = d["ctx"].shape[-1]
    B, Pn = d["qmask"].shape
    T = Pn * nq
    mem = d["memory"].transpose(0, 1)
    memp = (d["memory"] + d["pos"]).transpose(0, 1)
    q = R.qenc_forward(P, mem[:, :L], mem[:, 0], d["phrase"], d["ctx"], nq)
    qmask = d["qmask"][:, :, None].expand(-1, -1, nq).reshape(B, T)
    t, tq, qpos = q["tgt"].view(B, T, -1), q["tgtq"].view(B, T, -1), q["qpos"].view(B, T, -1)
    layers = []
    for i in range(ocfg.dec_layers):
        r = R.decoder_layer(P, f"{VT}decoder.layers.{i}.", t, t, tq, qpos, mem, memp, qmask, d["kpm"], ocfg.nheads)
        layers.append(r)
        t, tq = r["t3"], r["t3q"]
    t3 = torch.stack([r["t3"] for r in layers])                    # [NL, B, T, E]
    h = R.head_forward(P, t3)
    return dict(q=q, layers=layers, t3=t3, head=h, logits=h["logits"].view(len(layers), B, Pn, nq, 4), valid=~qmask)


def _weights(ocfg):
    wd, NL = O.weight_dict(ocfg), ocfg.dec_layers
    sfx = lambda l: "" if l == NL - 1 else f"_{l}"        # noqa: E731
    return torch.tensor([[wd["loss_bbox" + sfx(l)], wd["loss_giou" + sfx(l)]] for l in range(NL)], dtype=torch.float64)


def _oracle_losses(logits, valid, targets, ocfg):
    boxes = logits.sigmoid()
    out = {"pred_boxes": boxes[-1], "phrase_mask": valid,
           "aux_outputs": [{"pred_boxes": b, "phrase_mask": valid} for b in boxes[:-1]]}
    losses = O.criterion(out, targets)
    return losses, O.total_loss(losses, O.weight_dict(ocfg))


@pytest.mark.parametrize("B,L,HW,Pn,nq,pad", [(2, 9, 12, 1, 1, False), (3, 7, 10, 3, 1, True), (2, 8, 6, 2, 2, True)])
def test_free_running_stages_reproduce_the_oracle(small, B, L, HW, Pn, nq, pad):
    _, P0 = small
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), n_q=nq)
    d = _inputs(B, L, HW, Pn, nq, seed=B * 10 + Pn, pad_phrase=pad)
    res = {}
    for side in ("oracle", "stages"):
        P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
        if nq != 1:
            P["query_encoder.query_embed.weight"] = torch.randn(nq, 512, generator=torch.Generator().manual_seed(3),
                                                                 dtype=torch.float64).requires_grad_(True)
        dd = dict(d)
        for k in ("memory", "pos", "phrase"):
            dd[k] = d[k].clone().requires_grad_(True)
        f = _oracle_forward(P, dd, ocfg, nq) if side == "oracle" else _stage_forward(P, dd, ocfg, nq)
        losses, total = _oracle_losses(f["logits"], f["valid"], d["targets"], ocfg)
        leaves = {**{k: dd[k] for k in ("memory", "pos", "phrase")}, **P}
        grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
        res[side] = (f, losses, total, dict(zip(leaves, grads)))
    (fo, lo, to, go), (fs, ls, ts, gs) = res["oracle"], res["stages"]
    T = Pn * nq
    bm = lambda x: x.transpose(0, 1)        # noqa: E731  (the oracle is sequence-first)
    outs = {"tgt": (fs["q"]["tgt"].view(B, T, -1), bm(fo["tgt"])), "qpos": (fs["q"]["qpos"].view(B, T, -1), bm(fo["qpos"])),
            "hs": (fs["head"]["hs"].view(-1), fo["hs"].reshape(-1)), "logits": (fs["logits"], fo["logits"]), "total": (ts, to)}
    for i, r in enumerate(fs["layers"]):
        outs[f"t3[{i}]"] = (r["t3"], bm(fo["ts"][i]))
    # the stage functions' own loss rows and d total / d logits against the oracle's criterion and its autograd
    nb = max(sum(len(t["labels"]) for t in d["targets"]), 1.0)
    hl, htot, hdl = R.head_losses(fs["logits"].detach(), fs["valid"], d["targets"], nb, _weights(ocfg))
    NL = ocfg.dec_layers
    for l in range(NL):
        sfx = "" if l == NL - 1 else f"_{l}"
        outs[f"loss_bbox{sfx}"] = (hl[l, 0], lo["loss_bbox" + sfx])
        outs[f"loss_giou{sfx}"] = (hl[l, 1], lo["loss_giou" + sfx])
    outs["head_losses.total"] = (htot, to)
    lg = fo["logits"].detach().clone().requires_grad_(True)
    outs["dlogits"] = (hdl, torch.autograd.grad(_oracle_losses(lg, fo["valid"], d["targets"], ocfg)[1], lg)[0])
    worst = {}
    for k, (a, b) in outs.items():
        worst[k] = rel(a.detach(), b.detach())
        assert worst[k] <= TOL, (k, worst[k])
    # gradients.  One of them is zero in exact arithmetic and rounding noise on both sides, so it is held to noise size, not to the
    # other side: linear2.bias (the softmax is shift-invariant).
    noise = {"query_encoder.linear2.bias": "query_encoder.linear3.bias"}
    for k in go:
        if go[k] is None or gs[k] is None:
            assert go[k] is None and gs[k] is None, k
            continue
        if k in noise:
            assert max(float(go[k].norm()), float(gs[k].norm())) <= TOL * float(go[noise[k]].norm()), k
            continue
        worst["d " + k] = rel(gs[k], go[k])
        assert worst["d " + k] <= TOL, (k, worst["d " + k])
    print(f"\n[region_ref vs oracle B={B} L={L} P={Pn} nq={nq}] worst output {max(v for k, v in worst.items() if not k.startswith('d ')):.1e}"
          f"  worst gradient {max(v for k, v in worst.items() if k.startswith('d ')):.1e}")


@pytest.mark.parametrize("B,L,Pn,nq,drop,with_gb", [(2, 9, 1, 1, False, False), (3, 7, 4, 1, True, True), (2, 8, 3, 2, True, True)])
def test_query_encoder_backward_stages_equal_autograd(small, B, L, Pn, nq, drop, with_gb):
    _, P0 = small
    pfx = "query_encoder."
    g = torch.Generator().manual_seed(11 + B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    E, N = 256, B * Pn
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items() if k.startswith(pfx)}
    if nq != 1:
        P[pfx + "query_embed.weight"] = rn(nq, 2 * E).requires_grad_(True)
    lang, cls32, phrase = rn(B, L, E).requires_grad_(True), rn(B, E).requires_grad_(True), (0.5 * rn(B, Pn, E)).requires_grad_(True)
    ctx = torch.rand(B, Pn, L, generator=g) < 0.4
    ctx[:, :, 0] = False
    keep, p = (torch.rand(N, E, generator=g) >= 0.1, 0.1) if drop else (None, 0.0)
    f = R.qenc_forward(P, lang, cls32, phrase, ctx, nq, keep, p)
    ga, gb, dqpos = rn(N * nq, E), (rn(N * nq, E) if with_gb else None), rn(N * nq, E)
    obj = (f["tgt"] * (ga if gb is None else ga + gb)).sum() + (f["qpos"] * dqpos).sum()
    leaves = {"lang": lang, "cls32": cls32, "phrase": phrase, **P}
    ref = dict(zip(leaves, torch.autograd.grad(obj, list(leaves.values()))))
    fd = {k: v.detach() for k, v in f.items()}
    Pd = {k: v.detach() for k, v in P.items()}
    b = R.qenc_backward(Pd, fd, ga, gb, dqpos, nq, gate5=fd["f"] > 0, gate1=fd["y1"] > 0, keep=keep, p=p)
    wg = lambda dy, x: dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])        # noqa: E731
    cs = lambda dy: dy.reshape(-1, dy.shape[-1]).sum(0)        # noqa: E731
    dlang = b["dlang"].clone()
    dlang[:, 0] += b["dcls_lin"]
    cat = torch.cat([fd["cat_left"], phrase.detach()], -1).reshape(N, 2 * E)
    got = {"lang": dlang, "cls32": b["dcls_res"], "phrase": b["dcat"][:, E:].reshape(B, Pn, E), pfx + "query_embed.weight": b["dqembed"]}
    for name, dy, x in (("fuse_encoder_query.4.", b["dt2"], fd["a"]), ("fuse_encoder_query.0.", b["dt1"], cat),
                        ("context_out.0.", b["dco"], fd["c"]), ("linear1.", b["dk"], lang.detach()[:, 0]),
                        ("linear2.", b["dqs"], lang.detach()), ("linear3.", b["dvs"], lang.detach())):
        got[pfx + name + "weight"], got[pfx + name + "bias"] = wg(dy, x), cs(dy)
    for name, dy, x in (("fuse_encoder_query.5.", b["df"] * (fd["f"] > 0), fd["t2"]), ("fuse_encoder_query.1.", b["dy1"], fd["t1"]),
                        ("context_out.1.", b["dcat"][:, :E], fd["co"].reshape(N, E))):
        dgr, dbr = R.ln_param_rows(dy, x)
        got[pfx + name + "weight"], got[pfx + name + "bias"] = dgr.sum(0), dbr.sum(0)
    assert set(got) == set(ref)
    for k in ref:
        if k == pfx + "linear2.bias":       # zero in exact arithmetic (shift-invariant softmax): noise on both sides
            assert max(float(got[k].norm()), float(ref[k].norm())) <= TOL * float(ref[pfx + "linear3.bias"].norm())
            continue
        assert rel(got[k].reshape(ref[k].shape), ref[k]) <= TOL, (k, rel(got[k].reshape(ref[k].shape), ref[k]))


@pytest.mark.parametrize("B,Pn,nq", [(2, 1, 1), (3, 4, 1), (2, 2, 2)])
def test_head_backward_stages_equal_autograd(small, B, Pn, nq):
    ocfg, P0 = small
    NL, E = ocfg.dec_layers, 256
    g = torch.Generator().manual_seed(5 + Pn)
    norm, mlp = VT + "decoder.norm.", "bbox_embed.layers."
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items() if k.startswith((norm, mlp))}
    valid = torch.rand(B, Pn, generator=g) < 0.7
    valid[0, 0] = True
    if B > 2:
        valid[2] = False                    # an image without a valid phrase
    valid = valid[:, :, None].expand(-1, -1, nq).reshape(B, Pn * nq)
    nt = [int(v) // nq for v in valid.sum(1)]
    targets = [{"boxes": 0.3 + 0.4 * torch.rand(n, 4, generator=g, dtype=torch.float64), "labels": torch.zeros(n, dtype=torch.long)} for n in nt]
    nb = max(float(sum(nt)), 1.0)
    t3 = torch.randn(NL, B, Pn * nq, E, generator=g, dtype=torch.float64).requires_grad_(True)
    f = R.head_forward(P, t3)
    logits = f["logits"].view(NL, B, Pn, nq, 4)
    _, total = _oracle_losses(logits, valid, targets, ocfg)
    leaves = {"t3": t3, **P}
    ref = dict(zip(leaves, torch.autograd.grad(total, list(leaves.values()))))
    fd = {k: v.detach().reshape(NL * B * Pn * nq, -1) for k, v in f.items()}
    Pd = {k: v.detach() for k, v in P.items()}
    losses, tot, dl = R.head_losses(logits.detach(), valid, targets, nb, _weights(ocfg))
    assert abs(float(tot) - float(total.detach())) <= TOL * abs(float(total.detach()))
    dl = dl.reshape(-1, 4)
    assert float(dl.view(NL, B, Pn * nq, 4)[:, ~valid].abs().sum()) == 0.0      # invalid phrases: exactly zero
    b = R.head_backward(Pd, dict(t3=t3.detach().reshape(-1, E), y1=fd["y1"], y2=fd["y2"]), dl, Pd[mlp + "2.weight"])
    got = {"t3": b["dnorm"], norm + "weight": b["dgamma_rows"].sum(0), norm + "bias": b["dbeta_rows"].sum(0),
           mlp + "2.weight": dl.t() @ fd["y2"], mlp + "2.bias": dl.sum(0), mlp + "1.weight": b["dy2"].t() @ fd["y1"],
           mlp + "1.bias": b["dy2"].sum(0), mlp + "0.weight": b["dy1"].t() @ fd["hs"], mlp + "0.bias": b["dy1"].sum(0)}
    assert set(got) == set(ref)
    for k in ref:
        assert rel(got[k].reshape(ref[k].shape), ref[k]) <= TOL, (k, rel(got[k].reshape(ref[k].shape), ref[k]))
