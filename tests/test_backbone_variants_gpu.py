"""GPU: RefTR with the ResNeXt / Wide ResNet backbones (models/modeling/backbone.py:112-125 builds them by torchvision name) on
shallow configurations -- forward and gradients against the q-oracle (the HIP path's rounding points) with the grouped
convolutions of the oracle expressed as F.conv2d(groups=G), a captured step against the eager one, and the single-rank
data-parallel schedule against the plain step."""
import socket

import pytest
import torch
import torch.distributed as dist

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state

pytestmark = pytest.mark.gpu

PFX = "img_backbone.0.body."
VARIANTS = {"resnext50_32x4d": (32, 4), "resnext101_64x4d": (64, 4), "wide_resnet50_2": (1, 128)}
LAYERS = (1, 2, 1, 1)


def rel(a, b):
    a = torch.as_tensor(a).detach().float().cpu(); b = torch.as_tensor(b).detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def to_cuda(samples, targets):
    from reftr_amd.util.misc import NestedTensor
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].cuda(), samples["img_mask"].cuda())
    return s, [{k: v.cuda() for k, v in t.items()} for t in targets]


@pytest.fixture()
def grouped_oracle(monkeypatch):
    """The oracle's convolutions with groups = Cin / weight's Cin (1 for every dense convolution)."""
    orig = O.conv2d_acc

    def conv2d_acc(x, w, b=None, *a, **k):
        g = x.shape[1] // w.shape[1]
        if g > 1:
            k = dict(k, groups=g)
        return orig(x, w, b, *a, **k)
    monkeypatch.setattr(O, "conv2d_acc", conv2d_acc)


def build_variant(name, dilation=False, masks=False):
    from reftr_amd.models import layout as L
    from reftr_amd.models.reftr_transformer import RefTR
    groups, wpg = VARIANTS[name]
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), resnet_layers=LAYERS, dilation=dilation, masks=masks,
                 aux_loss=not masks)
    cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), resnet_layers=LAYERS, dilation=dilation, masks=masks,
                        aux_loss=not masks, resnet_groups=groups, resnet_width_per_group=wpg)
    shapes = dict(param_shapes(ocfg))
    for n, s, _ in L.resnet_table(PFX, LAYERS, True, groups, wpg):
        assert n in shapes
        shapes[n] = s
    P = formula_state(shapes)
    model = RefTR(cfg, device="cuda", aux_loss=not masks)
    model.load_state_dict(P, strict=True)
    model.eval()
    return model, P, ocfg


CASES = [("resnext50_32x4d", False), ("resnext50_32x4d", True), ("resnext101_64x4d", False), ("wide_resnet50_2", False),
         ("wide_resnet50_2", True)]


@pytest.mark.parametrize("name,dilation", CASES, ids=lambda v: str(v))
def test_variant_vs_q_oracle(hip, grouped_oracle, name, dilation):
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    model, P, ocfg = build_variant(name, dilation)
    crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
    samples, targets = make_inputs("e2e_single", B=2, H=128, W=160, L=12)
    s, tg = to_cuda(samples, targets)
    out = model(s)
    keys = [PFX + "layer2.0.conv2.weight", PFX + "layer4.0.conv2.weight", PFX + "layer3.0.conv1.weight", PFX + "layer2.1.conv3.weight",
            PFX + "layer4.0.downsample.0.weight", "input_proj.0.0.weight", "vl_transformer.encoder.layers.0.linear1.weight"]
    Pq = {k: v.clone() for k, v in P.items()}
    leaves = [Pq[k].requires_grad_(True) for k in keys]
    oq = O.reftr_forward(Pq, samples, ocfg, q=True)
    assert rel(out["pred_logits"].sigmoid().reshape(-1), oq["logits"].sigmoid().reshape(-1)) < 5e-3
    assert rel(out["pred_boxes"], oq["pred_boxes"]) < 5e-3
    lq = O.total_loss(O.criterion(oq, targets), O.weight_dict(ocfg))
    gq = torch.autograd.grad(lq, leaves)
    ld = crit(out, tg)
    total = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
    assert abs(float(total) - float(lq)) < 5e-3 * abs(float(lq))
    model.store.flat_g.zero_()
    total.backward()
    P2 = {k: v.clone() for k, v in P.items()}
    leaves2 = [P2[k].requires_grad_(True) for k in keys]
    with O.accumulate_fp64():
        o2 = O.reftr_forward(P2, samples, ocfg, q=True)
        g2 = torch.autograd.grad(O.total_loss(O.criterion(o2, targets), O.weight_dict(ocfg)), leaves2)
    report = []
    for k, q_, f_ in zip(keys, gq, g2):
        mine = model.store.G[k].float().cpu().reshape(q_.shape)
        report.append((k, rel(mine, q_), rel(f_.float(), q_)))
    print(f"\n[{name} dilation={dilation}] gradient rel-L2 vs q-oracle (HIP | fp64-order floor):")
    for r in report:
        print("   %-55s %.3e | %.3e" % r)
    for k, got, floor in report:
        assert got < max(1.5 * floor, 3e-2), (k, got, floor)


def test_resnext_seg_vs_q_oracle(hip, grouped_oracle):
    """--masks: the RES head reads the layer2 / layer3 outputs of the grouped backbone (and sends gradients back into them)."""
    from reftr_amd.models.criterion import CriterionVGOnePhraseSeg
    model, P, ocfg = build_variant("resnext50_32x4d", masks=True)
    wd = O.weight_dict(ocfg)
    crit = CriterionVGOnePhraseSeg(wd, losses=["masks", "boxes"])
    H, W = 128, 160
    samples, targets = make_inputs("seg_single", B=2, H=H, W=W, L=12)
    sizes = [(H, W), ((H * 3) // 4, (W * 2) // 3)]                  # image 1 carries right / bottom padding (oracle/synth.py)
    for t, (h, w) in zip(targets, sizes):
        m = torch.zeros(1, h, w, dtype=torch.bool)
        m[:, h // 5:(3 * h) // 4, w // 4:(4 * w) // 5] = True
        t["masks"] = m
    s, tg = to_cuda(samples, targets)
    out = model(s)
    keys = [PFX + "layer2.0.conv2.weight", PFX + "layer3.0.conv2.weight", PFX + "layer4.0.conv2.weight", "mask_head.adapter1.weight"]
    Pq = {k: v.clone() for k, v in P.items()}
    leaves = [Pq[k].requires_grad_(True) for k in keys]
    oq = O.reftr_forward(Pq, samples, ocfg, q=True)
    assert rel(out["pred_boxes"], oq["pred_boxes"]) < 5e-3
    lq = O.total_loss(O.criterion(oq, targets), wd)
    gq = torch.autograd.grad(lq, leaves)
    ld = crit(out, tg)
    total = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
    assert abs(float(total) - float(lq)) < 5e-3 * abs(float(lq))
    model.store.flat_g.zero_()
    total.backward()
    P2 = {k: v.clone() for k, v in P.items()}
    leaves2 = [P2[k].requires_grad_(True) for k in keys]
    with O.accumulate_fp64():
        o2 = O.reftr_forward(P2, samples, ocfg, q=True)
        g2 = torch.autograd.grad(O.total_loss(O.criterion(o2, targets), wd), leaves2)
    # the RES head's attention-map gradients are ill-conditioned (benchmarks/debug_seg_grads.py): 2 x the floor in rel-L2, the gate of
    # tests/test_seg_gpu.py
    for k, q_, f_ in zip(keys, gq, g2):
        mine = model.store.G[k].float().cpu().reshape(q_.shape)
        got, floor = rel(mine, q_), rel(f_.float(), q_)
        assert got < max(2.0 * floor, 3e-2), (k, got, floor)


def test_resnext_captured_step_matches_eager(hip, monkeypatch):
    from reftr_amd.engine_vg import CapturedTrainStep, train_step
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.optim import FusedAdamW
    monkeypatch.setenv("REFTR_HEAD_FUSE", "0")           # the eager loop's head kernel, as tests/test_model_gpu.py compares
    samples, targets = make_inputs("e2e_single", B=2, H=128, W=160, L=12)
    s, tg = to_cuda(samples, targets)
    runs = []
    for mode in ("eager", "graph"):
        model, P, ocfg = build_variant("resnext50_32x4d")
        crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
        opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
        if mode == "graph":
            p0, m0, v0 = model.store.flat_p.clone(), opt.m.clone(), opt.v.clone()
            cap = CapturedTrainStep(model, crit, opt, 0.1, s, tg, warmup=1)
            cap.reset_pending()
            model.store.flat_p.copy_(p0); opt.m.copy_(m0); opt.v.copy_(v0); opt.step_dev.zero_(); opt.step_count = 0
            model.mark_dirty(full=True)
            l, _, gn = cap(s, tg)
            lv = float(l)
        else:
            lv, _, _, gn = train_step(model, crit, s, tg, opt, None, max_norm=0.1)
        torch.cuda.synchronize()
        g = model.store.flat_g.clone()
        # the clip norm (collected where the gradients are produced, grouped weight gradients included) is the buffer's norm
        assert abs(float(gn) - float(g.double().norm())) < 1e-4 * float(g.double().norm()), (mode, float(gn), float(g.norm()))
        if mode == "graph":
            cap.flush()
        runs.append((lv, float(gn), g, model.store.flat_p.clone()))
    (l0, n0, g0, p0_), (l1, n1, g1, p1_) = runs
    assert abs(l0 - l1) < 1e-6 * abs(l0) and abs(n0 - n1) < 1e-5 * n0, (l0, l1, n0, n1)
    assert rel(g1, g0) < 1e-6 and rel(p1_, p0_) < 1e-7


def _free_port():
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); p = sk.getsockname()[1]; sk.close()
    return p


def test_resnext_single_rank_dp_schedule_follows_the_plain_step(hip, monkeypatch):
    from reftr_amd.engine_vg import train_step
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.optim import FusedAdamW
    from reftr_amd.parallel import DistributedDataParallel
    monkeypatch.setenv("REFTR_DDP_FORCE", "1")
    monkeypatch.setenv("REFTR_DDP_DTYPE", "fp32")
    samples, targets = make_inputs("e2e_single", B=2, H=128, W=160, L=12)
    s, tg = to_cuda(samples, targets)
    out = {}
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", world_size=1, rank=0)
    try:
        for mode in ("eager", "dp"):
            model, P, ocfg = build_variant("resnext50_32x4d")
            crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
            opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
            runner = DistributedDataParallel(model) if mode == "dp" else model
            if mode == "dp":
                assert runner.active and model.dp_mode
            lv, _, _, gn = train_step(runner, crit, s, tg, opt, None, max_norm=0.1)
            torch.cuda.synchronize()
            out[mode] = (lv, float(gn), model.store.flat_g.clone(), model.store.flat_p.clone())
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    (l0, n0, g0, p0), (l1, n1, g1, p1) = out["eager"], out["dp"]
    assert abs(l1 - l0) < 1e-6 * abs(l0)
    assert rel(g1, g0) < 1e-6 and abs(n1 - n0) < 1e-5 * n0
    assert rel(p1, p0) < 1e-7
