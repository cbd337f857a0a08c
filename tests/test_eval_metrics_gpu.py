"""GPU: the device evaluation metrics (csrc/rt_eval.hip through hip.eval_metrics / metrics.EvalMeter) against util/box_ops.py and
plain torch ops on the same device, and engine_vg.evaluate with the meter against its per-image torch loop.

Exactness: the kernel issues box_ops' fp32 operations un-fused in box_ops' order, so iou_det carries the bits of
diag(box_iou(...)); the mask counts are integers; the hit counts compare the same fp32 values against the same fp32 thresholds.
The two double sums add fp32 values one by one in double: against the correctly rounded float64 sum (math.fsum) of the same
values that is at most (n - 1) roundings of 2^-53 relative for non-negative terms, plus fsum's own one -> n * 2^-53.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import reftr_oracle as O
from oracle.shapes import param_shapes
from oracle.synth import make_inputs
from oracle.weights import formula_state

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = (0.5, 0.6, 0.7, 0.8, 0.9)
NEW_KEYS = {"seg_oiou"} | {f"seg_prec@{t}" for t in THR}


def _hits(v):
    """Samples strictly above the fp32 value nearest each threshold (a NaN is a miss)."""
    return [int((v > torch.tensor(t, dtype=torch.float32, device=v.device)).sum()) for t in THR]


def _slots(acc):
    h = acc.cpu()
    return h[:14].tolist() + h[14:].view(torch.float64).tolist()


def _close_sum(got, values, n):
    want = math.fsum(float(v) for v in values.double().cpu().tolist())
    return abs(got - want) <= n * 2.0 ** -53 * abs(want), (got, want)


def _same_bits(a, b):
    """NaNs in the same places, every other value bit for bit."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


def _table(hip, targets, sizes=None):
    from reftr_amd.metrics import build_table
    words, keep = build_table(targets, sizes)
    dev = words.cuda()
    B = len(targets)
    return dev[:5 * B].view(B, 5), (dev[5 * B:].view(torch.int32).view(B, 2) if sizes is not None else None), keep


def _ref_box_ious(pred, valid, tboxes):
    """Per image diag(box_iou(target, the valid phrases' prediction 0)) with util/box_ops.py on the device."""
    from reftr_amd.util import box_ops
    out = []
    for b, tb in enumerate(tboxes):
        sel = pred[b][valid[b]][:, 0][:tb.shape[0]]
        out.append(torch.diag(box_ops.box_iou(box_ops.box_cxcywh_to_xyxy(tb), box_ops.box_cxcywh_to_xyxy(sel))[0]))
    return out


PLANTED = [((0.4, 0.6, 0.25, 0.5), (0.4, 0.6, 0.25, 0.5)),        # identical: IoU 1
           ((0.2, 0.2, 0.2, 0.2), (0.8, 0.8, 0.2, 0.2)),          # disjoint: IoU 0
           ((0.5, 0.5, 1.0, 1.0), (0.5, 0.25, 1.0, 0.5)),         # IoU exactly 0.5: NOT a hit at 0.5
           ((0.3, 0.3, 0.0, 0.0), (0.3, 0.3, 0.0, 0.0))]          # zero area: 0 / 0 = NaN


def _box_case(B, P, K, seed, p_valid, empty, full, first_row):
    """Ragged validity with one image without a valid phrase and one with all valid; the planted pairs sit in the all-valid image
    from row `first_row` on (P = 70: rows 62..65, across the boundary of the kernel's 64-at-a-time walk)."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, P, K, 4, generator=g)
    valid = torch.rand(B, P, generator=g) < p_valid
    valid[empty] = False
    valid[full] = True
    tboxes = [torch.cat([torch.rand(int(valid[b].sum()), 2, generator=g), 0.05 + 0.5 * torch.rand(int(valid[b].sum()), 2, generator=g)], 1)
              for b in range(B)]
    for i, (gt, pr) in enumerate(PLANTED):
        tboxes[full][first_row + i] = torch.tensor(gt)
        pred[full, first_row + i, 0] = torch.tensor(pr)
    return pred.cuda(), valid.cuda(), [t.cuda() for t in tboxes]


@pytest.mark.parametrize("B,P,K,seed,p_valid,empty,full,first_row", [(5, 16, 2, 3, 0.5, 2, 4, 1), (3, 70, 1, 11, 0.4, 0, 1, 62)])
def test_box_iou_rows_hits_and_sum(hip, B, P, K, seed, p_valid, empty, full, first_row):
    pred, valid, tboxes = _box_case(B, P, K, seed, p_valid, empty, full, first_row)
    v8 = valid[:, :, None].expand(B, P, K).to(torch.uint8).contiguous()
    nan_row = first_row + 3
    for with_nan in (True, False):
        if not with_nan:                                # the zero-area pair becomes an ordinary one
            tboxes[full][nan_row] = torch.tensor([0.5, 0.5, 0.2, 0.3], device="cuda")
            pred[full, nan_row, 0] = torch.tensor([0.55, 0.5, 0.2, 0.3], device="cuda")
        table, _, keep = _table(hip, [{"boxes": t} for t in tboxes])
        acc = torch.full((hip.EVAL_SLOTS,), -7, dtype=torch.int64, device="cuda")          # reset: whatever it held is gone
        iou_det, iou_seg, iu = hip.eval_metrics(pred, v8, table, acc, reset=True)
        assert iou_seg is None and iu is None and iou_det.shape == (B, P)
        ref = _ref_box_ious(pred, valid, tboxes)
        for b, r in enumerate(ref):
            n = r.shape[0]
            assert n == int(valid[b].sum())
            assert _same_bits(iou_det[b, :n], r), (b, iou_det[b, :n], r)
            assert bool((iou_det[b, n:].view(torch.int32) == 0).all())                     # unused rows are +0.0
        allv = torch.cat(ref)
        row = iou_det[full, first_row:first_row + 4].tolist()
        assert row[0] == 1.0 and row[1] == 0.0 and row[2] == 0.5 and (math.isnan(row[3]) if with_nan else 0.0 < row[3] < 1.0)
        s = _slots(acc)
        assert s[hip.EVAL_DET_N] == allv.numel() == sum(t.shape[0] for t in tboxes)
        assert s[hip.EVAL_DET_HIT:hip.EVAL_DET_HIT + 5] == _hits(allv)
        assert s[hip.EVAL_SEG_N:hip.EVAL_SEG_U + 1] == [0] * 8 and s[hip.EVAL_SEG_SUM] == 0.0
        if with_nan:
            assert int(torch.isnan(allv).sum()) == 1 and math.isnan(s[hip.EVAL_DET_SUM])
        else:
            ok, info = _close_sum(s[hip.EVAL_DET_SUM], allv, allv.numel())
            assert ok, info


def test_box_rows_stop_at_the_target_count(hip):
    """At most n_b rows are read: a table that names fewer target boxes than the image has valid phrases scores only those."""
    pred, valid, tboxes = _box_case(5, 16, 2, 3, 0.5, 2, 4, 1)
    v8 = valid[:, :, None].expand(5, 16, 2).to(torch.uint8).contiguous()
    short = [t[:max(t.shape[0] - 2, 0)].contiguous() for t in tboxes]
    short[4] = short[4][:1]                                                 # in front of the planted NaN row
    table, _, keep = _table(hip, [{"boxes": t} for t in short])
    acc = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")
    iou_det, _, _ = hip.eval_metrics(pred, v8, table, acc, reset=True)
    ref = _ref_box_ious(pred, valid, short)
    for b, r in enumerate(ref):
        assert _same_bits(iou_det[b, :r.shape[0]], r) and bool((iou_det[b, r.shape[0]:] == 0).all())
    s = _slots(acc)
    assert s[hip.EVAL_DET_N] == sum(t.shape[0] for t in short) and s[hip.EVAL_DET_HIT:hip.EVAL_DET_HIT + 5] == _hits(torch.cat(ref))


MASK_SIZES = [(1, 1), (7, 13), (37, 61), (64, 64), (33, 257), (129, 517)]


def _mask_case(sizes, seed, Q=2, empty=None, forms=True):
    """Frame = the maximum size; pred is 1 OUTSIDE every image's own [:ih, :iw] (a read past the crop is counted and caught), inside it
    the target with a per-image share of flipped pixels (IoUs spread from 1 downwards); query 1 is noise (only query 0 is scored).
    Targets alternate [h, w] / [1, h, w] and bool / uint8."""
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    mh, mw = max(s[0] for s in sizes), max(s[1] for s in sizes)
    frame = torch.ones(B, Q, mh, mw, dtype=torch.uint8)
    frame[:, 1:] = (torch.rand(B, Q - 1, mh, mw, generator=g) < 0.5).to(torch.uint8)
    targets = []
    for b, (h, w) in enumerate(sizes):
        t = torch.rand(h, w, generator=g) < 0.6
        t[0, 0] = True                                   # never an empty union by chance (the 1 x 1 image)
        p = t ^ (torch.rand(h, w, generator=g) < 0.04 * b)
        if b == empty:
            t[:] = False; p[:] = False
        frame[b, 0, :h, :w] = p.to(torch.uint8)
        m = t if (b % 2 == 0 or not forms) else t[None]
        m = m.to(torch.uint8) * 3 if (b // 2) % 2 == 1 and forms else m                     # any non-zero byte is a set pixel
        targets.append({"boxes": torch.tensor([[0.5, 0.5, 0.2, 0.2]]).cuda(), "masks": m.cuda()})
    return frame.cuda(), targets


def _ref_masks(frame, targets, sizes):
    inter, union = [], []
    for b, (h, w) in enumerate(sizes):
        p, t = frame[b, 0, :h, :w].bool(), targets[b]["masks"].reshape(h, w) != 0
        inter.append(torch.sum(torch.logical_and(p, t))); union.append(torch.sum(torch.logical_or(p, t)))
    inter, union = torch.stack(inter), torch.stack(union)
    return inter, union, inter.float() / union.float()                                      # util/box_ops.py mask_iou


def _trivial_boxes(B):
    pred = torch.tensor([0.5, 0.5, 0.2, 0.2], device="cuda").repeat(B, 1, 1, 1).contiguous()
    return pred, torch.ones(B, 1, 1, dtype=torch.uint8, device="cuda")


def test_mask_counts_iou_and_hits(hip):
    """Six sizes in one frame of 129 x 517; with RT_EVAL_CHUNK = 16384 pixels per workgroup the last image (66693 pixels) spans five
    chunks, (33, 257) = 8481 pixels and the smaller ones a part of one."""
    sizes = MASK_SIZES
    assert hip.EVAL_CHUNK == 16384 and sizes[-1][0] * sizes[-1][1] > 4 * hip.EVAL_CHUNK
    frame, targets = _mask_case(sizes, seed=21, empty=1)
    assert {(t["masks"].dim(), t["masks"].dtype) for t in targets} == {(2, torch.bool), (3, torch.bool), (2, torch.uint8), (3, torch.uint8)}
    B = len(sizes)
    table, sizes_dev, keep = _table(hip, targets, sizes)
    pred, v8 = _trivial_boxes(B)
    acc = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")
    iou_det, iou_seg, iu = hip.eval_metrics(pred, v8, table, acc, masks=frame, sizes_i32=sizes_dev, reset=True)
    inter, union, ref = _ref_masks(frame, targets, sizes)
    assert iu.dtype == torch.int64 and torch.equal(iu[:, 0], inter) and torch.equal(iu[:, 1], union)
    assert int(union[1]) == 0 and int(torch.isnan(ref).sum()) == 1 and bool(torch.isnan(iou_seg[1]))       # empty against empty
    assert _same_bits(iou_seg, ref), (iou_seg, ref)
    assert float(ref[0]) == 1.0 and float(ref[-1]) < 0.9                                    # a spread of IoUs: the hit counts differ
    s = _slots(acc)
    assert s[hip.EVAL_SEG_N] == B and s[hip.EVAL_SEG_I] == int(inter.sum()) and s[hip.EVAL_SEG_U] == int(union.sum())
    assert s[hip.EVAL_SEG_HIT:hip.EVAL_SEG_HIT + 5] == _hits(ref) and len(set(_hits(ref))) > 1
    assert math.isnan(s[hip.EVAL_SEG_SUM])                                                  # the NaN sample, as torch's running sum
    assert s[hip.EVAL_DET_N] == B and s[hip.EVAL_DET_HIT] == B and s[hip.EVAL_DET_SUM] == float(B)


def test_accumulation_reset_and_determinism(hip):
    """Three updates of different batches = one computation over their concatenation; reset; two identical runs, identical bits."""
    from reftr_amd.metrics import EvalMeter
    cases = []
    for (B, P, K, seed, first), sizes in zip([(5, 16, 2, 3, 1), (3, 70, 1, 11, 62), (2, 16, 2, 5, 0)],
                                             [[(37, 61), (64, 64), (33, 257), (7, 13), (129, 517)], [(129, 517), (1, 1), (64, 64)], [(7, 13), (37, 61)]]):
        pred, valid, tboxes = _box_case(B, P, K, seed, 0.5, 0, B - 1, first)
        tboxes[B - 1][first + 3] = torch.tensor([0.5, 0.5, 0.2, 0.3], device="cuda")       # no NaN row: the sums are checked
        pred[B - 1, first + 3, 0] = torch.tensor([0.55, 0.5, 0.2, 0.3], device="cuda")
        frame, targets = _mask_case(sizes, seed=seed + 100, forms=(seed != 11))
        for t, bx in zip(targets, tboxes):
            t["boxes"] = bx
        out = {"pred_boxes": pred, "phrase_mask": valid[:, :, None].expand(B, P, K).reshape(B, P * K)}
        cases.append((out, targets, frame, sizes, valid, tboxes))

    def run():
        meter = EvalMeter("cuda")
        meter.acc.fill_(123456789)                      # the first update resets inside its own launch
        meter._fresh = True
        for out, targets, frame, sizes, _, _ in cases:
            meter.update(out, targets, masks=frame, sizes=sizes)
        return meter
    meter = run()
    det = torch.cat([torch.cat(_ref_box_ious(o["pred_boxes"], v, tb)) for o, _, _, _, v, tb in cases])
    refs = [_ref_masks(f, t, s) for _, t, f, s, _, _ in cases]
    inter, union, seg = (torch.cat([r[i] for r in refs]) for i in range(3))
    s = _slots(meter.acc)
    assert s[hip.EVAL_DET_N] == det.numel() and s[hip.EVAL_DET_HIT:hip.EVAL_DET_HIT + 5] == _hits(det)
    assert s[hip.EVAL_SEG_N] == seg.numel() == 10 and s[hip.EVAL_SEG_HIT:hip.EVAL_SEG_HIT + 5] == _hits(seg)
    assert s[hip.EVAL_SEG_I] == int(inter.sum()) and s[hip.EVAL_SEG_U] == int(union.sum())
    for slot, vals in ((hip.EVAL_DET_SUM, det), (hip.EVAL_SEG_SUM, seg)):
        ok, info = _close_sum(s[slot], vals, vals.numel())
        assert ok, (slot, info)
    # `last` is the last batch's
    assert _same_bits(meter.last.iou_seg, refs[-1][2]) and torch.equal(meter.last.iu[:, 0], refs[-1][0])
    assert meter.last.iou_det.shape == (2, 16)
    stats = meter.compute()
    assert stats["seg_oiou"] == int(inter.sum()) / int(union.sum()) and stats["seg_miou"] == s[hip.EVAL_SEG_SUM] / 10
    assert stats["seg_prec@0.7"] == _hits(seg)[2] / 10 and stats["miou"] == s[hip.EVAL_DET_SUM] / det.numel()
    # the same again: the same bits
    again = run()
    assert torch.equal(again.acc, meter.acc) and torch.equal(again.last.iou_det.view(torch.int32), meter.last.iou_det.view(torch.int32))
    # reset: every slot zero, and the statistics of nothing
    meter.reset()
    assert _slots(meter.acc) == [0] * 14 + [0.0, 0.0]
    z = meter.compute()
    assert z["accuracy_iou0.5"] == 0.0 and z["miou"] == 0.0


def test_argument_checks(hip):
    import ctypes
    pred, v8 = _trivial_boxes(2)
    table, _, keep = _table(hip, [{"boxes": torch.zeros(1, 4, device="cuda")} for _ in range(2)])
    acc = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")
    iou = torch.zeros(2, 1, device="cuda")

    def call(**kw):
        f = dict(pred_boxes=pred.data_ptr(), valid=v8.data_ptr(), table=table.data_ptr(), iou_det=iou.data_ptr(), acc=acc.data_ptr(),
                 B=2, P=1, K=1, reset=1)
        f.update(kw)
        return hip.lib().rt_eval_metrics(ctypes.byref(hip.EvalMetricsArgs(**f)), torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    for name in ("pred_boxes", "valid", "table", "iou_det", "acc"):
        assert call(**{name: None}) == -1, name                               # RT_ERR_BADARG
    for name in ("B", "P", "K"):
        assert call(**{name: 0}) == -1, name
    seg = dict(masks=v8.data_ptr(), sizes=v8.data_ptr(), partials=v8.data_ptr(), iou_seg=v8.data_ptr(), iu=v8.data_ptr(), Q=1)
    assert call(**seg, max_h=0, max_w=4) == -1 and call(**dict(seg, sizes=None), max_h=4, max_w=4) == -1
    assert call(**seg, max_h=1 << 16, max_w=1 << 15) == -2                    # RT_ERR_UNSUPPORTED: 2^31 pixels; nothing is launched
    torch.cuda.synchronize()


def test_box_postprocess_unchanged_by_the_shared_ranking(hip):
    """rt_box_postprocess now ranks through the helper it shares with rt_eval_metrics: the ragged multi-query case and the P > 64
    case of tests/test_post_gpu.py stay bit-identical to the oracle, scaled and unscaled, and so do the counts."""
    for seed, (B, P, K), p_valid, sizes in ((3, (5, 16, 2), 0.5, [[480, 640], [333, 500], [640, 427], [1, 1], [799, 1333]]),
                                            (11, (3, 150, 1), 0.4, [[480, 640], [333, 500], [640, 427]])):
        g = torch.Generator().manual_seed(seed)
        pred = torch.rand(B, P, K, 4, generator=g)
        valid = torch.rand(B, P, generator=g) < p_valid
        if B == 5:
            valid[2] = False; valid[4] = True
        else:
            valid[1] = True
        mask = valid[:, :, None].expand(B, P, K).reshape(B, P * K)
        sizes = torch.tensor(sizes)
        v8 = mask.reshape(B, P, K).to(torch.uint8).cuda().contiguous()
        for scale in (False, True):
            out, counts = hip.box_postprocess(pred.cuda(), v8, sizes.float().cuda() if scale else None)
            ref = O.postprocess_boxes(pred, mask, sizes, scale)
            assert counts.tolist() == [int(v.sum()) for v in valid]
            for b, r in enumerate(ref):
                assert torch.equal(out[b, :r.shape[0]].cpu().view(torch.int32), r.view(torch.int32)), (seed, scale, b)
                assert bool((out[b, r.shape[0]:] == 0).all())


# ---------------------------------------------------------------- end to end

def _to_cuda(samples, targets):
    from reftr_amd.util.misc import NestedTensor
    s = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"].cuda(), samples["img_mask"].cuda())
    return s, [{k: v.cuda() for k, v in t.items()} for t in targets]


def _build(masks):
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase, CriterionVGOnePhraseSeg
    from reftr_amd.models.reftr_transformer import RefTR
    if masks:
        ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), masks=True, aux_loss=False)
        cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), masks=True)
        model = RefTR(cfg, device="cuda", aux_loss=False)
        crit = CriterionVGOnePhraseSeg(O.weight_dict(ocfg), ["masks", "boxes"])
    else:
        ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2))
        cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2))
        model = RefTR(cfg, device="cuda")
        crit = CriterionVGMultiPhrase(O.weight_dict(ocfg), ["boxes"])
    model.load_state_dict(formula_state(param_shapes(ocfg)), strict=True)
    return model, crit


def _loader(samples, targets, n):
    from reftr_amd.util.misc import NestedTensor
    s = {k: v for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"], samples["img_mask"])
    return [(s, targets)] * n


def test_evaluate_metered_against_the_torch_loop(hip, monkeypatch):
    """The two-batch RES loader of tests/test_seg_gpu.py::test_evaluate_rec_and_res_metrics, REFTR_EVAL_METRICS=1 against =0.
    (The losses of the two runs are compared for equality: the mask-loss forward adds its workgroups' partial sums in a fixed order,
    hip.mask_loss's workspace -- through fp32 atomics loss_dice moved by an ulp from one run to the next.)"""
    import torch.nn.functional as F
    from reftr_amd.engine_vg import evaluate
    from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase
    g = np.load(os.path.join(GOLD, "seg_single.npz"))
    model, crit = _build(masks=True)
    samples, targets = make_inputs("seg_single", B=2, H=96, W=128, L=12)
    targets = [dict(t, masks=torch.from_numpy(g[f"target_mask{i}"])) for i, t in enumerate(targets)]
    for i, t in enumerate(targets):
        h, w = t["masks"].shape[-2:]
        t.update(size=torch.tensor([h, w]), orig_size=torch.tensor([2 * h + 1, 3 * w]), image_id=torch.tensor(10 + i),
                 dataset_id=torch.tensor(i))
    loader = _loader(samples, targets, 2)
    post = {"bbox": PostProcessVGMultiPhrase(), "segm": PostProcessSegm()}
    run = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("REFTR_EVAL_METRICS", switch)
        run[switch] = evaluate(model, crit, post, loader, torch.device("cuda"))
    (new, res_new), (old, res_old) = run["1"], run["0"]
    assert not (NEW_KEYS & set(old)) and NEW_KEYS <= set(new) and set(new) - NEW_KEYS == set(old)
    assert new["accuracy_iou0.5"] == old["accuracy_iou0.5"]
    for k in ("miou", "seg_miou"):                      # the loop's fp32 running sum against the meter's double
        assert abs(new[k] - old[k]) <= 1e-6 * abs(old[k]), (k, new[k], old[k])
    for k in old:
        if k.startswith("loss"):
            assert new[k] == old[k], k
    assert res_new == res_old and set(res_new) == {10, 11} and len(res_new[10]) == 1 and len(res_new[10][0]) == 4
    assert all(type(v) is float for v in res_new[10][0])
    # the new keys against a recomputation in torch from the model's outputs
    model.eval()
    cs, ct = _to_cuda(samples, targets)
    with torch.no_grad():
        out = model(cs)
    pm = F.interpolate(out["pred_masks"].squeeze(2), size=tuple(torch.stack([t["size"] for t in targets]).max(0)[0].tolist()),
                       mode="bilinear", align_corners=False).sigmoid() > 0.5
    I = U = 0
    ious = []
    for i, t in enumerate(ct):
        h, w = t["masks"].shape[-2:]
        p, m = pm[i, 0, :h, :w], t["masks"][0]
        a, b = int(torch.logical_and(p, m).sum()), int(torch.logical_or(p, m).sum())
        I += a; U += b
        ious.append(torch.tensor(a).float() / torch.tensor(b).float())
    ious = torch.stack(ious).cuda()
    assert abs(new["seg_oiou"] - (2 * I) / (2 * U)) <= 1e-12 * new["seg_oiou"]              # two passes over the same batch
    for t, hits in zip(THR, _hits(ious)):
        assert abs(new[f"seg_prec@{t}"] - (2 * hits) / 4) <= 1e-12, t
    assert abs(new["seg_miou"] - float(ious.double().mean())) <= 1e-6 * new["seg_miou"]


def test_evaluate_rec_only_has_no_mask_keys(hip, monkeypatch):
    """No 'segm' post-processor: no seg_* key; Acc@0.5 / mIoU of the multi-phrase model (3 and 2 valid phrases) against torch."""
    from reftr_amd.engine_vg import evaluate
    from reftr_amd.models.post_process import PostProcessVGMultiPhrase
    from reftr_amd.util import box_ops
    monkeypatch.delenv("REFTR_EVAL_METRICS", raising=False)
    model, crit = _build(masks=False)
    samples, targets = make_inputs("e2e_multi", B=2, H=96, W=128, L=12, n_phrase=3)
    for i, t in enumerate(targets):
        t.update(size=torch.tensor([96, 128]), orig_size=torch.tensor([200 + i, 300]), image_id=torch.tensor(20 + i))
    stats, results = evaluate(model, crit, {"bbox": PostProcessVGMultiPhrase()}, _loader(samples, targets, 2), torch.device("cuda"))
    assert not any(k.startswith("seg_") for k in stats) and {"accuracy_iou0.5", "miou", "loss"} <= set(stats)
    model.eval()
    cs, ct = _to_cuda(samples, targets)
    with torch.no_grad():
        out = model(cs)
    B, P, K, _ = out["pred_boxes"].shape
    valid = out["phrase_mask"].reshape(B, P, K)[:, :, 0].bool()
    assert valid.sum(1).tolist() == [3, 2]
    iou = torch.cat(_ref_box_ious(out["pred_boxes"].float(), valid, [t["boxes"] for t in ct]))
    assert stats["accuracy_iou0.5"] == float((iou > 0.5).float().sum() / 5)
    assert abs(stats["miou"] - float(iou.double().mean())) <= 1e-12 + 5 * 2.0 ** -53 * stats["miou"]
    assert set(results) == {20, 21} and [len(results[k]) for k in (20, 21)] == [3, 2]
