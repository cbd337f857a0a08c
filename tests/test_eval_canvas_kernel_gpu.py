"""GPU: rt_eval_canvas / rt_eval_facts (csrc/rt_eval.hip, csrc/rt_post.hip) against the three launches they replace on the same tensors:
hip.mask_postprocess with the canvas as frame + hip.box_postprocess scaled to the original sizes + hip.eval_metrics.

Every comparison is exact: the mask counts are integers taken from the same decision function compiled in the same file, the box
arithmetic is un-fused fp32 in one order, the sums are added in one order.  NaNs (0 / 0) must sit in the same places.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


class Batch:
    """One synthetic canvas batch on the device: model-side tensors (pred_boxes, valid, pred_masks), loader-side targets, and the
    buffers rt_batch_stage / rt_eval_facts fill."""

    def __init__(self, hip, canvas, logit_hw, sizes, P, K, valid_rows, n_tgt, seed, Q=2, tmask="rand", logits=None, static=None):
        g = torch.Generator().manual_seed(seed)
        self.hip, (self.Hc, self.Wc), self.B, self.P, self.K = hip, canvas, len(sizes), P, K
        B, (h, w) = self.B, logit_hw
        self.sizes = [tuple(s) for s in sizes]
        self.orig = [(2 * ih + 1, 3 * iw) for ih, iw in sizes]
        self.pred_boxes = torch.rand(B, P, K, 4, generator=g).cuda()
        valid = torch.zeros(B, P, dtype=torch.bool)
        for b, rows in enumerate(valid_rows):
            valid[b, list(rows)] = True
        self.valid = valid[:, :, None].expand(B, P, K).to(torch.uint8).contiguous().cuda()
        self.pred_masks = (torch.randn(B, Q, h, w, generator=g) if logits is None else logits).float().contiguous().cuda()
        self.targets = []
        for b, (ih, iw) in enumerate(sizes):
            mode = tmask[b] if isinstance(tmask, (list, tuple)) else tmask
            m = {"rand": torch.rand(1, ih, iw, generator=g) < 0.5, "zero": torch.zeros(1, ih, iw, dtype=torch.bool),
                 "one": torch.ones(1, ih, iw, dtype=torch.bool)}[mode]
            bx = torch.cat([torch.rand(n_tgt[b], 2, generator=g), 0.05 + 0.5 * torch.rand(n_tgt[b], 2, generator=g)], 1)
            self.targets.append({"boxes": bx.cuda(), "masks": (m.to(torch.uint8) * 3).cuda(),
                                 "size": torch.tensor([ih, iw]).cuda(), "orig_size": torch.tensor(self.orig[b]).cuda(),
                                 "image_id": torch.tensor(1000 * seed + b).cuda()})
        self.static = static if static is not None else self.alloc()
        self.stage()

    def alloc(self):
        B, Hc, Wc, P = self.B, self.Hc, self.Wc, self.P
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        return dict(img=z((B, 3, Hc, Wc), torch.float32), mask=z((B, Hc, Wc), torch.uint8), boxes=z((B * P, 4), torch.float32),
                    tgt_off=z(B + 1, torch.int32), nb=z(1, torch.float32), tgt_masks=z((B, 1, Hc, Wc), torch.uint8),
                    facts=z((B, 6), torch.int32), ids=z(B, torch.int64))

    def stage(self):
        """What the evaluation loop issues per batch: rt_batch_stage (a 1 x 1 image: the model side is synthetic) + rt_eval_facts."""
        s, hip, B = self.static, self.hip, self.B
        hip.batch_stage(torch.zeros(B, 3, 1, 1, device="cuda"), torch.zeros(B, 1, 1, dtype=torch.uint8, device="cuda"), s["img"], s["mask"],
                        [t["boxes"] for t in self.targets], self.P, s["boxes"], s["tgt_off"], s["nb"],
                        mask_list=[t["masks"] for t in self.targets], tgt_masks=s["tgt_masks"])
        hip.eval_facts([t["size"] for t in self.targets], s["facts"], s["ids"], origs=[t["orig_size"] for t in self.targets],
                       ids=[t["image_id"] for t in self.targets], mask_hw=[t["masks"].shape[-2:] for t in self.targets])

    def reference(self, acc, reset):
        """The three existing launches; returns (iou_det, iou_seg, iu, scaled boxes [B, P, 4], counts)."""
        from reftr_amd.metrics import build_table
        hip, B = self.hip, self.B
        sizes_i32 = torch.tensor(self.sizes, dtype=torch.int32).cuda()
        frame, _ = hip.mask_postprocess(self.pred_masks, sizes_i32, (self.Hc, self.Wc))
        out, counts = hip.box_postprocess(self.pred_boxes, self.valid, torch.tensor(self.orig, dtype=torch.float32).cuda())
        words, keep = build_table(self.targets, self.sizes)
        dev = words.cuda()
        r = hip.eval_metrics(self.pred_boxes, self.valid, dev[:5 * B].view(B, 5), acc, masks=frame,
                             sizes_i32=dev[5 * B:].view(torch.int32).view(B, 2), reset=reset)
        torch.cuda.synchronize()
        return (*r, out, counts)

    def canvas(self, state, **kw):
        s = self.static
        return self.hip.eval_canvas(self.pred_boxes, self.valid, s["boxes"], s["tgt_off"], s["facts"], s["ids"], state,
                                    pred_masks=self.pred_masks, tgt_masks=s["tgt_masks"], **kw)


def _check_against_reference(hip, batch):
    acc_ref = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")
    det_r, seg_r, iu_r, boxes_r, counts_r = batch.reference(acc_ref, reset=True)
    state = hip.EvalCanvasState(2, batch.B, batch.P, "cuda")
    det, seg, iu = batch.canvas(state)
    torch.cuda.synchronize()
    assert _same_bits(det, det_r), (det, det_r)
    assert _same_bits(seg, seg_r), (seg, seg_r)
    assert torch.equal(iu, iu_r), (iu, iu_r)
    assert torch.equal(state.acc, acc_ref), (state.acc, acc_ref)                           # all 16 slots, raw int64
    assert state.cursor.tolist() == [1, 0]
    assert torch.equal(state.boxes[0].view(torch.int32), boxes_r.view(torch.int32))
    assert torch.equal(state.counts[0], counts_r) and torch.equal(state.ids[0], batch.static["ids"])
    assert state.ids[0].tolist() == [int(t["image_id"]) for t in batch.targets]
    assert bool((state.boxes[1] == 0).all()) and bool((state.counts[1] == 0).all())        # the next slot is untouched
    return seg, iu


def test_two_chunks_unaligned_pitch_and_the_second_phrase_pass(hip):
    """Canvas 150 x 130 (19500 pixels: two chunks of 16384, Wc neither a multiple of 4 nor of 16), logits 25 x 33.  Sizes: the full canvas
    (its first chunk ends inside row 126), one row, one column, 127 x 129 = 16383 pixels (one short of a chunk).  P = 70, K = 1: image 0's
    first valid phrase is index 62, its others lie in the second 64-lane pass; image 1 has no target box, image 2 no valid phrase, image
    3 more valid phrases than targets."""
    assert hip.EVAL_CHUNK == 16384
    b = Batch(hip, (150, 130), (25, 33), [(150, 130), (1, 130), (150, 1), (127, 129)], P=70, K=1,
              valid_rows=[(62, 65, 69), (3, 64), (), (0, 10, 63, 64, 68)], n_tgt=[3, 0, 2, 3], seed=5, tmask="rand")
    _check_against_reference(hip, b)


def test_one_exact_chunk_and_target_mask_extremes(hip):
    """Canvas 128 x 128 = exactly one chunk, logits 32 x 32, P = 16, K = 2.  Target masks: all-zero, all-one, random, and all-zero
    against logits that are all negative (empty against empty: 0 / 0 = NaN in iou_seg and in the running sum, as today)."""
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(4, 2, 32, 32, generator=g)
    logits[3, 0] = -5.0
    b = Batch(hip, (128, 128), (32, 32), [(128, 128), (64, 96), (128, 1), (100, 128)], P=16, K=2,
              valid_rows=[(0, 1, 2), (5,), (1, 15), (2, 3)], n_tgt=[3, 1, 2, 2], seed=7, tmask=["zero", "one", "rand", "zero"], logits=logits)
    seg, iu = _check_against_reference(hip, b)
    assert iu[0, 0] == 0 and iu[0, 1] > 0 and float(seg[0]) == 0.0          # target empty inside [:ih, :iw], prediction not
    assert iu[3].tolist() == [0, 0] and bool(torch.isnan(seg[3]))           # both empty
    assert iu[1, 1] == 64 * 96                                              # the all-one target: the union is the scored rectangle


def _axis64(n_out, n_in):
    """torch's bilinear source index and weight (align_corners=False) in float64."""
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def _bilinear64(lg, Hc, Wc):
    y0, y1, ly = _axis64(Hc, lg.shape[0])
    x0, x1, lx = _axis64(Wc, lg.shape[1])
    ly, lx = ly[:, None], lx[None, :]
    a, b, c, d = lg[y0][:, x0], lg[y0][:, x1], lg[y1][:, x0], lg[y1][:, x1]
    return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)


def _borderline_logits(h, w, Hc, Wc, seed):
    """Logits whose float64 bilinear interpolant vanishes (up to the fp32 rounding of one logit) at one frame pixel strictly inside
    every third source cell: the fourth corner of the cell is solved in float64 and rounded to fp32."""
    rng = np.random.default_rng(seed)
    lg = rng.uniform(-1.0, 1.0, size=(h, w)).astype(np.float32).astype(np.float64)
    y0, _, ly = _axis64(Hc, h)
    x0, _, lx = _axis64(Wc, w)
    for cy in range(0, h - 1, 3):
        for cx in range(0, w - 1, 3):
            ys = [y for y in range(Hc) if y0[y] == cy and 0.0 < ly[y] < 1.0]
            xs = [x for x in range(Wc) if x0[x] == cx and 0.0 < lx[x] < 1.0]
            if not ys or not xs:
                continue
            y, x = max(ys, key=lambda v: ly[v]), max(xs, key=lambda v: lx[v])
            a, b, c = lg[cy, cx], lg[cy, cx + 1], lg[cy + 1, cx]
            d = -((1 - ly[y]) * ((1 - lx[x]) * a + lx[x] * b) + ly[y] * (1 - lx[x]) * c) / (ly[y] * lx[x])
            lg[cy + 1, cx + 1] = np.float64(np.float32(d))
    return lg


@pytest.mark.parametrize("hw,canvas", [((24, 32), (96, 128)), ((25, 33), (150, 130)), ((40, 36), (160, 144))])
def test_borderline_pixels_take_the_post_processors_decision(hip, hw, canvas):
    """Per image at least 64 scored pixels whose float64 interpolant is below 2^-20 in magnitude: one fused multiply-add more or less
    in the interpolation flips the decision on several of them, so the canvas kernel agrees with rt_mask_postprocess on every image
    only if both compile the decision under one contraction setting.  The count is asserted (a condition on the input)."""
    (h, w), (Hc, Wc) = hw, canvas
    B, Q = 4, 2
    logits = torch.zeros(B, Q, h, w, dtype=torch.float64)
    for b in range(B):
        lg = _borderline_logits(h, w, Hc, Wc, seed=100 * h + b)
        near = int((np.abs(_bilinear64(lg, Hc, Wc)) < 2.0 ** -20).sum())
        assert near >= 64, (b, near)
        logits[b, 0] = torch.from_numpy(lg)
    logits[:, 1] = torch.randn(B, h, w, dtype=torch.float64)
    bt = Batch(hip, canvas, hw, [canvas] * B, P=16, K=2, valid_rows=[(0,), (1,), (2,), (3,)], n_tgt=[1, 1, 1, 1], seed=h,
               tmask="rand", logits=logits.float())
    assert torch.equal(bt.pred_masks[:, 0].double().cpu(), logits[:, 0])                 # the solved logits are fp32 values
    _check_against_reference(hip, bt)


def _three(hip, static=None):
    specs = [dict(sizes=[(150, 130), (20, 31)], valid_rows=[(0, 2), (1,)], n_tgt=[2, 1], seed=21),
             dict(sizes=[(3, 5), (149, 129)], valid_rows=[(), (4, 5, 6)], n_tgt=[0, 3], seed=22),
             dict(sizes=[(77, 130), (150, 64)], valid_rows=[(7,), (0, 15)], n_tgt=[1, 2], seed=23)]
    return [dict(canvas=(150, 130), logit_hw=(25, 33), P=16, K=2, tmask="rand", static=static, **s) for s in specs]


def test_replay_of_one_graph_and_the_ring(hip):
    """Three different batches staged into one set of static buffers and replayed from ONE captured rt_eval_canvas give the
    accumulators of three eager calls; twice over, the same bits; the cursor ends at 3.  A ring of two slots raises the overflow word
    on the third batch, keeps the cursor at 2 and leaves the memory behind the ring as it was."""
    eager = hip.EvalCanvasState(3, 2, 16, "cuda")
    ref_acc = torch.zeros(hip.EVAL_SLOTS, dtype=torch.int64, device="cuda")
    rings = []
    for i, kw in enumerate(_three(hip)):
        b = Batch(hip, **kw)
        b.canvas(eager)
        *_, boxes_r, counts_r = b.reference(ref_acc, reset=(i == 0))
        rings.append((boxes_r, counts_r, b.static["ids"].clone()))
    torch.cuda.synchronize()
    assert torch.equal(eager.acc, ref_acc) and eager.cursor.tolist() == [3, 0]
    for i, (bx, cn, ids) in enumerate(rings):
        assert torch.equal(eager.boxes[i].view(torch.int32), bx.view(torch.int32)) and torch.equal(eager.counts[i], cn)
        assert torch.equal(eager.ids[i], ids)

    # one graph over static buffers; the per-batch work outside it is staging alone
    first = Batch(hip, **_three(hip)[0])
    static = first.static
    model_side = dict(pred_boxes=first.pred_boxes.clone(), valid=first.valid.clone(), pred_masks=first.pred_masks.clone())
    state = hip.EvalCanvasState(3, 2, 16, "cuda")
    first.pred_boxes, first.valid, first.pred_masks = model_side["pred_boxes"], model_side["valid"], model_side["pred_masks"]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = first.canvas(state)
    runs = []
    for _ in range(2):
        state.acc.zero_(); state.cursor.zero_(); state.boxes.fill_(-1.0)
        for kw in _three(hip, static=static):
            b = Batch(hip, **kw)                                   # stages into the static buffers
            for k, v in model_side.items():
                v.copy_(getattr(b, k))
            graph.replay()
        torch.cuda.synchronize()
        runs.append((state.acc.clone(), state.boxes.clone(), state.counts.clone(), state.ids.clone(), out[0].clone()))
        assert state.cursor.tolist() == [3, 0]
    assert torch.equal(runs[0][0], eager.acc)
    assert torch.equal(runs[0][1].view(torch.int32), eager.boxes.view(torch.int32)) and torch.equal(runs[0][2], eager.counts)
    assert torch.equal(runs[0][3], eager.ids)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)

    # a ring of two slots inside guarded memory
    small = hip.EvalCanvasState(2, 2, 16, "cuda")
    gb = torch.full((3, 2, 16, 4), 12345.0, device="cuda"); gc_ = torch.full((3, 2), 77, dtype=torch.int32, device="cuda")
    gi = torch.full((3, 2), -99, dtype=torch.int64, device="cuda")
    small.boxes, small.counts, small.ids = gb[:2], gc_[:2], gi[:2]
    accs = []
    for kw in _three(hip):
        Batch(hip, **kw).canvas(small)
        accs.append(small.acc.clone())
    torch.cuda.synchronize()
    assert small.cursor.tolist() == [2, 1]
    assert bool((gb[2] == 12345.0).all()) and bool((gc_[2] == 77).all()) and bool((gi[2] == -99).all())
    assert torch.equal(gb[:2].view(torch.int32), eager.boxes[:2].view(torch.int32)) and torch.equal(gc_[:2], eager.counts[:2])
    assert torch.equal(accs[2], eager.acc)                        # the totals do not depend on the ring


def test_veto_word_keeps_nothing_of_the_batch(hip):
    """A non-zero veto word: per-batch outputs are written, totals, ring and cursor stay as they were."""
    b = Batch(hip, **_three(hip)[0])
    state = hip.EvalCanvasState(2, 2, 16, "cuda")
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    det, seg, iu = b.canvas(state, veto=word)
    torch.cuda.synchronize()
    assert bool((state.acc == 0).all()) and state.cursor.tolist() == [0, 0] and bool((state.boxes == 0).all())
    word.zero_()
    det2, seg2, iu2 = b.canvas(state, veto=word)
    torch.cuda.synchronize()
    assert state.cursor.tolist() == [1, 0] and int(state.acc[hip.EVAL_SEG_N]) == 2
    assert _same_bits(det, det2) and _same_bits(seg, seg2) and torch.equal(iu, iu2)


@pytest.mark.parametrize("B", [1, 64])
def test_eval_facts_table(hip, B):
    assert B <= hip.BATCH_STAGE_MAX_B
    g = torch.Generator().manual_seed(B)
    size = torch.randint(1, 2000, (B, 2), generator=g)
    orig = torch.randint(1, 5000, (B, 2), generator=g)
    ids = torch.randint(0, 2 ** 53, (B,), generator=g)
    hw = [(int(a), int(b)) for a, b in torch.randint(1, 700, (B, 2), generator=g)]
    sz = [r.cuda() for r in size]; og = [r.cuda() for r in orig]; idl = [v.cuda() for v in ids]
    facts = torch.full((B, 6), -1, dtype=torch.int32, device="cuda"); out_ids = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    hip.eval_facts(sz, facts, out_ids, origs=og, ids=idl, mask_hw=hw)
    want = torch.cat([size, orig, torch.tensor(hw)], 1).to(torch.int32)
    assert torch.equal(facts.cpu(), want) and torch.equal(out_ids.cpu(), ids)
    hip.eval_facts(sz, facts, out_ids)                           # no orig_size: the size; no image_id: -1; no masks: 0
    assert torch.equal(facts.cpu(), torch.cat([size, size, torch.zeros(B, 2, dtype=torch.long)], 1).to(torch.int32))
    assert out_ids.tolist() == [-1] * B


def test_argument_checks(hip):
    b = Batch(hip, **_three(hip)[0])
    state = hip.EvalCanvasState(2, 2, 16, "cuda")
    s = b.static
    partials = torch.zeros(2, 2, 2, dtype=torch.int32, device="cuda"); det = torch.zeros(2, 16, device="cuda")
    seg = torch.zeros(2, device="cuda"); iu = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        f = dict(pred_boxes=b.pred_boxes.data_ptr(), valid=b.valid.data_ptr(), tgt_boxes=s["boxes"].data_ptr(), tgt_off=s["tgt_off"].data_ptr(),
                 facts=s["facts"].data_ptr(), image_ids=s["ids"].data_ptr(), pred_masks=b.pred_masks.data_ptr(),
                 tgt_masks=s["tgt_masks"].data_ptr(), partials=partials.data_ptr(), iou_det=det.data_ptr(), iou_seg=seg.data_ptr(),
                 iu=iu.data_ptr(), acc=state.acc.data_ptr(), ring_boxes=state.boxes.data_ptr(), ring_counts=state.counts.data_ptr(),
                 ring_ids=state.ids.data_ptr(), cursor=state.cursor.data_ptr(), B=2, P=16, K=2, Q=2, h=25, w=33, Hc=150, Wc=130,
                 tgt_rows=32, slots=2, threshold=0.5)
        f.update(kw)
        return hip.lib().rt_eval_canvas(ctypes.byref(hip.EvalCanvasArgs(**f)), stream)
    for name in ("pred_boxes", "valid", "tgt_boxes", "tgt_off", "facts", "image_ids", "iou_det", "acc", "ring_boxes", "ring_counts",
                 "ring_ids", "cursor", "tgt_masks", "partials", "iou_seg", "iu"):
        assert call(**{name: None}) == -1, name                                # RT_ERR_BADARG
    for name in ("B", "P", "K", "Q", "h", "w", "Hc", "Wc", "slots"):
        assert call(**{name: 0}) == -1, name
    assert call(B=hip.BATCH_STAGE_MAX_B + 1) == -2                             # RT_ERR_UNSUPPORTED
    assert call(Hc=1 << 16, Wc=1 << 15) == -2                                  # 2^31 pixels
    torch.cuda.synchronize()
    assert state.cursor.tolist() == [0, 0] and bool((state.acc == 0).all())    # nothing was launched
    # rt_eval_facts
    P8 = ctypes.c_void_p * 2
    sz = P8(b.targets[0]["size"].data_ptr(), b.targets[1]["size"].data_ptr())
    L = hip.lib()
    assert L.rt_eval_facts(None, None, None, None, 2, s["facts"].data_ptr(), s["ids"].data_ptr(), stream) == -1
    assert L.rt_eval_facts(sz, None, None, None, 2, None, s["ids"].data_ptr(), stream) == -1
    assert L.rt_eval_facts(sz, None, None, None, 0, s["facts"].data_ptr(), s["ids"].data_ptr(), stream) == -1
    assert L.rt_eval_facts(P8(sz[0], None), None, None, None, 2, s["facts"].data_ptr(), s["ids"].data_ptr(), stream) == -1
    assert L.rt_eval_facts(sz, None, None, None, hip.BATCH_STAGE_MAX_B + 1, s["facts"].data_ptr(), s["ids"].data_ptr(), stream) == -2
    torch.cuda.synchronize()
