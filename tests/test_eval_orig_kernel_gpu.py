"""GPU: rt_eval_raw_facts / rt_eval_orig (csrc/rt_eval.hip, csrc/rt_post.hip) alone, against rt_mask_postprocess's masks_origin with
the canvas as the frame (test_predict_kernel_gpu.oracle_masks, query 0) combined with the raw target bytes by torch integer sums, and
the host formulas for the accumulators.

Every comparison is exact: the counts are integers taken from the one decision function compiled in one file, the IoU is one
correctly rounded fp32 division, the running sum adds the fp32 values in image order in double.
"""
import numpy as np
import pytest
import torch

from reftr_amd import hip as H
from test_eval_canvas_kernel_gpu import _bilinear64, _borderline_logits
from test_predict_kernel_gpu import FIVE, oracle_masks

pytestmark = pytest.mark.gpu

CANVAS, LOGIT_HW, Q = (96, 128), (24, 32), 2
SIX = FIVE + [((96, 128), (130, 150))]           # 19500 pixels: two chunks, the smallest image that crosses a chunk boundary
POISON = -77                                     # (a partial is a count: never negative)
THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


def make_logits(B, seed, borderline=()):
    """Random logits [B, Q, 24, 32]; query 0 of the images in `borderline` is _borderline_logits' plane: at least 64 canvas pixels
    whose float64 interpolant is below 2^-20 in magnitude, so one fused multiply-add more or less flips decisions."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, Q, *LOGIT_HW, generator=g, dtype=torch.float64)
    for b in borderline:
        lg = _borderline_logits(*LOGIT_HW, *CANVAS, seed=100 * seed + b)
        assert int((np.abs(_bilinear64(lg, *CANVAS)) < 2.0 ** -20).sum()) >= 64
        logits[b, 0] = torch.from_numpy(lg)
    return logits.float().contiguous().cuda()


def make_targets(origs, seed, zero=()):
    """One flat uint8 device tensor per image, bytes drawn from {0, 1, 2, 255} (all zero for the images in `zero`)."""
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)
    return [(torch.zeros(oh * ow, dtype=torch.uint8) if b in zero else values[torch.randint(0, 4, (oh * ow,), generator=g)]).cuda()
            for b, (oh, ow) in enumerate(origs)]


def expected(hip, logits, sizes, origs, targets, scored=None, thr=0.5):
    """(iu int64 [B, 2], iou_seg fp32 [B], the RT_EVAL_ORIG_SLOTS values this batch adds) by the definition, on the host."""
    B = len(origs)
    iu = torch.zeros(B, 2, dtype=torch.int64)
    for b, (blk, (oh, ow)) in enumerate(zip(oracle_masks(hip, logits, sizes, origs, CANVAS, thr), origs)):
        if scored is not None and not scored[b]:
            continue
        pred, tgt = blk[:oh * ow] != 0, targets[b] != 0                               # query 0; a non-zero byte is set
        iu[b, 0], iu[b, 1] = int((pred & tgt).sum()), int((pred | tgt).sum())
    iou = iu[:, 0].float() / iu[:, 1].float()                                         # fp32 division, 0 / 0 = NaN
    n, hits, total = 0, [0] * 5, 0.0
    for b in range(B):
        if scored is not None and not scored[b]:
            iou[b] = 0.0
            continue
        n += 1
        for k, t in enumerate(THRESHOLDS):
            hits[k] += int(bool(iou[b] > torch.tensor(t, dtype=torch.float32)))
        total += float(iou[b])                                                        # (double += fp32, in image order)
    return iu, iou, [n, *hits, int(iu[:, 0].sum()), int(iu[:, 1].sum()), total]


def slots_of(acc):
    host = acc.cpu()
    return host[:H.EVAL_ORIG_SUM].tolist() + host[H.EVAL_ORIG_SUM:].view(torch.float64).tolist()


def same_slots(got, want):
    assert got[:8] == want[:8], (got, want)
    assert got[8] == want[8] or (np.isnan(got[8]) and np.isnan(want[8])), (got, want)


def same_bits(a, b):
    return bool(torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)))


def run(hip, logits, sizes, origs, targets, ids=None, veto=None, acc=None, max_pixels=None, zero_entries=(), thr=0.5):
    """rt_eval_raw_facts + rt_eval_orig on a state whose partials start from POISON -> (state, facts, image_ids)."""
    B = len(origs)
    max_pixels = max(oh * ow for oh, ow in origs) if max_pixels is None else max_pixels
    st = hip.EvalOrigState(B, max_pixels, "cuda", acc=acc)
    st.partials.fill_(POISON); st.iou_seg.fill_(-3.0); st.iu.fill_(-5)
    facts = torch.full((B, 6), -9, dtype=torch.int32, device="cuda")
    image_ids = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    hip.eval_raw_facts(sizes, origs, CANVAS, facts, image_ids, ids=ids, mask_list=targets, mask_table=st.mask_table, max_pixels=max_pixels)
    for b in zero_entries:
        st.mask_table[b] = 0
    hip.eval_orig(logits, facts, st, CANVAS, threshold=thr, veto=veto)
    torch.cuda.synchronize()
    return st, facts, image_ids


def check_partials(hip, st, origs, scored=None):
    """Slots behind each image's own chunk count keep the poison; the image's own slots add up to its iu."""
    part, iu = st.partials.cpu(), st.iu.cpu()
    for b, (oh, ow) in enumerate(origs):
        mine = -(-(oh * ow) // hip.EVAL_CHUNK) if scored is None or scored[b] else 0
        assert bool((part[b, mine:] == POISON).all()), b
        assert not bool((part[b, :mine] == POISON).any()), b
        assert part[b, :mine].to(torch.int64).sum(0).tolist() == iu[b].tolist(), b


def test_six_images_every_branch_and_the_chunk_boundary(hip):
    sizes, origs = [s for s, _ in SIX], [o for _, o in SIX]
    logits = make_logits(6, 3, borderline=(0, 1, 5))
    targets = make_targets(origs, 4)
    st, facts, image_ids = run(hip, logits, sizes, origs, targets, ids=[10, 11, 12, 1 << 40, 14, 15])
    assert st.partials.shape[1] == 11 and 333 * 500 == 166500                          # the grid: 11 chunks per image, most leave at once
    # rt_eval_raw_facts: the rows, the ids and the table are the host values
    assert facts.cpu().tolist() == [[*s, *o, *s] for s, o in SIX]
    assert image_ids.cpu().tolist() == [10, 11, 12, 1 << 40, 14, 15]
    assert st.mask_table.cpu().tolist() == [t.data_ptr() for t in targets]
    iu, iou, slots = expected(hip, logits, sizes, origs, targets)
    assert torch.equal(st.iu.cpu(), iu) and same_bits(st.iou_seg, iou)
    same_slots(slots_of(st.acc), slots)
    assert all(0 < int(i) < int(u) for i, u in iu[[0, 1, 2, 3, 5]].tolist()) and slots[0] == 6      # (a condition on the input)
    check_partials(hip, st, origs)
    assert -(-(130 * 150) // hip.EVAL_CHUNK) == 2 and bool((st.partials[5, :2, 1] > 0).all())
    # a second run: the same bits, and the accumulators add up (never reset by the kernel)
    again, _, ids2 = run(hip, logits, sizes, origs, targets, acc=st.acc)
    assert torch.equal(again.iu, st.iu) and same_bits(again.iou_seg, st.iou_seg) and torch.equal(again.partials, st.partials)
    assert ids2.cpu().tolist() == [-1] * 6                                             # without ids
    twice = slots_of(st.acc)
    assert twice[:8] == [2 * v for v in slots[:8]]
    total = 0.0
    for v in iou.tolist() * 2:
        total += v
    assert twice[8] == total


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base_plus_1"])
def test_mask_base_alignment_and_the_guard_byte(hip, shift):
    """The raw masks at a 16-byte-aligned base and at base + 1 (every unit takes the byte loads), each followed directly by a guard byte
    of 255: the counts are those of the aligned masks without a guard -- the oracle's."""
    pairs = [((96, 128), (37, 51)), ((24, 32), (1, 17)), ((48, 64), (96, 128)), ((75, 100), (130, 150))]     # h * w % 16: 15, 1, 0, 12
    sizes, origs = [s for s, _ in pairs], [o for _, o in pairs]
    logits = make_logits(4, 7, borderline=(2,))
    plain = make_targets(origs, 8)
    placed, keep = [], []
    for t in plain:
        buf = torch.full((t.numel() + 32,), 255, dtype=torch.uint8, device="cuda")    # poison all round
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + t.numel()] = t
        keep.append(buf)
        placed.append(buf[shift:shift + t.numel()])
        assert placed[-1].data_ptr() % 16 == shift and int(buf[shift + t.numel()]) == 255
    st, _, _ = run(hip, logits, sizes, origs, placed)
    iu, iou, slots = expected(hip, logits, sizes, origs, plain)
    assert torch.equal(st.iu.cpu(), iu) and same_bits(st.iou_seg, iou)
    same_slots(slots_of(st.acc), slots)
    check_partials(hip, st, origs)


def test_empty_against_empty_is_nan_and_a_miss(hip):
    sizes, origs = [(96, 128), (75, 100), (48, 64)], [(130, 150), (75, 100), (96, 128)]
    logits = make_logits(3, 9)
    logits[1, 0] = -5.0                                                                # no pixel of image 1 is predicted
    targets = make_targets(origs, 10, zero=(1,))
    st, _, _ = run(hip, logits, sizes, origs, targets)
    iu, iou, slots = expected(hip, logits, sizes, origs, targets)
    assert iu[1].tolist() == [0, 0] and bool(torch.isnan(iou[1])) and np.isnan(slots[8]) and slots[0] == 3
    assert torch.equal(st.iu.cpu(), iu) and bool(torch.isnan(st.iou_seg[1])) and same_bits(st.iou_seg[[0, 2]], iou[[0, 2]])
    got = slots_of(st.acc)
    same_slots(got, slots)
    assert got[0] == 3 and np.isnan(got[8]) and got[1] <= 2                            # counted, a miss, and the sum is NaN


def test_veto_leaves_the_accumulators_alone(hip):
    sizes, origs = [(96, 128), (75, 100)], [(130, 150), (37, 51)]
    logits, targets = make_logits(2, 11), make_targets(origs, 12)
    acc = torch.arange(100, 100 + hip.EVAL_ORIG_SLOTS, dtype=torch.int64, device="cuda")
    before = acc.clone()
    veto = torch.tensor([3], dtype=torch.int32, device="cuda")
    st, _, _ = run(hip, logits, sizes, origs, targets, veto=veto, acc=acc)
    iu, iou, slots = expected(hip, logits, sizes, origs, targets)
    assert torch.equal(acc, before)                                                    # vetoed: not one slot moved
    assert torch.equal(st.iu.cpu(), iu) and same_bits(st.iou_seg, iou)                 # ... the batch's own outputs are written
    veto.zero_()
    acc.zero_()
    st, _, _ = run(hip, logits, sizes, origs, targets, veto=veto, acc=acc)
    same_slots(slots_of(acc), slots)


def test_a_zero_table_entry_leaves_the_image_out(hip):
    sizes, origs = [(96, 128), (75, 100), (48, 64)], [(130, 150), (333, 500), (96, 128)]
    logits, targets = make_logits(3, 13), make_targets(origs, 14)
    scored = [True, False, True]
    st, _, _ = run(hip, logits, sizes, origs, targets, zero_entries=(1,))
    iu, iou, slots = expected(hip, logits, sizes, origs, targets, scored=scored)
    assert torch.equal(st.iu.cpu(), iu) and st.iu[1].tolist() == [0, 0] and float(st.iou_seg[1]) == 0.0 and same_bits(st.iou_seg, iou)
    same_slots(slots_of(st.acc), slots)
    assert slots[0] == 2
    check_partials(hip, st, origs, scored=scored)                                      # image 1: every slot keeps the poison


def test_a_grid_sized_for_more_pixels_than_any_image_has(hip):
    """max_pixels = 16 x the canvas, as the evaluation step sizes it: 12 chunks per image here, of which an image uses its own."""
    sizes, origs = [(24, 32), (96, 128)], [(1, 17), (130, 150)]
    logits, targets = make_logits(2, 15, borderline=(1,)), make_targets(origs, 16)
    st, _, _ = run(hip, logits, sizes, origs, targets, max_pixels=16 * CANVAS[0] * CANVAS[1])
    assert st.partials.shape[1] == 12
    iu, iou, slots = expected(hip, logits, sizes, origs, targets)
    assert torch.equal(st.iu.cpu(), iu) and same_bits(st.iou_seg, iou)
    same_slots(slots_of(st.acc), slots)
    check_partials(hip, st, origs)
