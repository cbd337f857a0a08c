"""GPU: rt_predict_facts / rt_predict_canvas (csrc/rt_predict.hip, csrc/rt_post.hip) against the two launches they replace on the same
tensors: hip.box_postprocess scaled to the original sizes and the masks_origin of hip.mask_postprocess with the canvas as its frame.

Every comparison is bit for bit and leaves no element out: the mask decision is one function compiled in one file, the box
arithmetic is un-fused fp32 in one order.  The packed buffer is compared whole -- blocks, zero tails and guard bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_eval_canvas_kernel_gpu import _bilinear64, _borderline_logits

pytestmark = pytest.mark.gpu

POISON = 0xA5


def oracle_masks(hip, logits, sizes, origs, canvas, thr=0.5):
    """masks_origin of rt_mask_postprocess, frame = canvas: one flat uint8 tensor per image ([Q, orig_h, orig_w] flattened)."""
    B, Q = logits.shape[:2]
    off = [0]
    for oh, ow in origs:
        off.append(off[-1] + Q * oh * ow)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    _, packed = hip.mask_postprocess(logits, i32(sizes), canvas, thr, orig_i32=i32(origs), origin_off=torch.tensor(off).cuda(),
                                     origin_total=off[-1], max_origin=max(oh * ow for oh, ow in origs))
    return [packed[off[b]:off[b + 1]] for b in range(B)]


def expected_buffer(hip, before, logits, sizes, origs, canvas, thr=0.5):
    """The mask buffer after a call: `before` with [0, 16 * off16[B]) replaced by the oracle's blocks and their zero tails."""
    Q = logits.shape[1]
    off = hip.predict_layout(Q, origs)
    want = before.clone()
    want[:16 * off[-1]] = 0
    for b, blk in enumerate(oracle_masks(hip, logits, sizes, origs, canvas, thr)):
        want[16 * off[b]:16 * off[b] + blk.numel()] = blk
    return want, off


def guarded_state(hip, B, P, capacity, behind=64):
    """A PredictState whose mask buffer has `behind` more bytes than the capacity the kernels are told."""
    st = hip.PredictState(B, P, "cuda", mask_capacity=capacity + behind)
    assert capacity % 16 == 0 and st.capacity == capacity + behind
    st.capacity = capacity
    st.block.fill_(POISON)
    return st


def boxes_and_valid(B, P, K, valid_rows, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, P, K, 4, generator=g).cuda()
    valid = torch.zeros(B, P, dtype=torch.bool)
    for b, rows in enumerate(valid_rows):
        valid[b, list(rows)] = True
    return pred, valid[:, :, None].expand(B, P, K).to(torch.uint8).contiguous().cuda()


def check_boxes(hip, st, pred, valid, origs):
    out, counts = hip.box_postprocess(pred, valid, torch.tensor(origs, dtype=torch.float32).cuda())
    assert torch.equal(st.out_boxes.view(torch.int32), out.view(torch.int32)) and torch.equal(st.out_counts, counts)


FIVE = [((75, 100), (75, 100)),          # the identity branch
        ((48, 64), (96, 128)),           # the exact-double branch
        ((75, 100), (333, 500)),         # generic up-scale, ow % 16 != 0
        ((96, 128), (37, 51)),           # down-scale; 2 * 37 * 51 = 3774 bytes: a zero tail of 2
        ((24, 32), (1, 17))]             # 34 bytes: a block smaller than three units


def test_five_images_every_branch_tails_and_guards(hip):
    canvas, Q = (96, 128), 2
    sizes, origs = [s for s, _ in FIVE], [o for _, o in FIVE]
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(5, Q, 24, 32, generator=g).cuda()
    pred, valid = boxes_and_valid(5, 3, 2, [(0, 2), (), (0, 1, 2), (1,), (2,)], 12)
    total = hip.predict_layout(Q, origs)[-1]
    st = guarded_state(hip, 5, 3, 16 * total + 64)               # 64 guard bytes inside the capacity, 64 more behind it
    hip.predict_facts(sizes, origs, canvas, st.facts, Q=Q, capacity=st.capacity)
    before = st.masks.clone()
    hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)
    torch.cuda.synchronize()
    want, off = expected_buffer(hip, before, logits, sizes, origs, canvas)
    assert off[-1] == total and 16 * off[4] - 16 * off[3] - 3774 == 2
    facts = st.facts.cpu()
    assert facts[:, :4].tolist() == [[*s, *o] for s, o in FIVE] and facts[:, 4].tolist() == off[:-1] and facts[:, 5].tolist() == off[1:]
    assert facts[:, 6].tolist() == [total] * 5 and facts[:, 7].tolist() == [0] * 5
    assert torch.equal(st.masks, want)                                                 # blocks, zero tails, guards: every byte
    assert bool((st.masks[16 * total:] == POISON).all()) and st.masks.numel() == 16 * total + 128
    assert not bool((st.masks[:16 * total] == POISON).any())                           # every byte below the total was rewritten
    for b in range(5):
        end = 16 * off[b] + Q * origs[b][0] * origs[b][1]
        assert bool((st.masks[end:16 * off[b + 1]] == 0).all())
    assert 0 < int(st.masks[:16 * total].sum()) < 16 * total
    check_boxes(hip, st, pred, valid, origs)
    # a second, smaller batch into the same buffer: nothing at or past ITS total changes
    sizes2, origs2 = [(60, 80), (96, 128)], [(33, 47), (96, 128)]
    logits2 = torch.randn(5, Q, 24, 32, generator=g).cuda()
    before = st.masks.clone()
    st2 = hip.PredictState(2, 3, "cuda")                                               # B = 2 over the same mask buffer
    st2.masks, st2.capacity = st.masks, st.capacity
    hip.predict_facts(sizes2, origs2, canvas, st2.facts, Q=Q, capacity=st2.capacity)
    hip.predict_canvas(pred[:2].contiguous(), valid[:2].contiguous(), st2, pred_masks=logits2[:2].contiguous(), canvas_hw=canvas)
    torch.cuda.synchronize()
    want2, off2 = expected_buffer(hip, before, logits2[:2].contiguous(), sizes2, origs2, canvas)
    assert off2[-1] < total and torch.equal(st.masks, want2)
    assert torch.equal(st.masks[16 * off2[-1]:], before[16 * off2[-1]:])
    check_boxes(hip, st2, pred[:2].contiguous(), valid[:2].contiguous(), origs2)


def test_capacity_bounds_the_writes_whatever_the_facts_say(hip):
    """Facts written for a large buffer, the kernel told a small one: nothing past the small capacity is touched; what lies below it
    is the oracle's."""
    canvas, Q, sizes, origs = (96, 128), 2, [(75, 100), (96, 128)], [(75, 100), (37, 51)]
    logits = torch.randn(2, Q, 24, 32, generator=torch.Generator().manual_seed(3)).cuda()
    pred, valid = boxes_and_valid(2, 3, 1, [(0,), (1, 2)], 4)
    total = hip.predict_layout(Q, origs)[-1]
    st = guarded_state(hip, 2, 3, 16 * total, behind=64)
    hip.predict_facts(sizes, origs, canvas, st.facts, Q=Q, capacity=st.capacity)
    before = st.masks.clone()
    want, _ = expected_buffer(hip, before, logits, sizes, origs, canvas)
    st.capacity = 16 * (total // 2)
    hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)
    torch.cuda.synchronize()
    assert torch.equal(st.masks[:st.capacity], want[:st.capacity]) and bool((st.masks[st.capacity:] == POISON).all())
    st.capacity = 16 * total                                   # exactly the total: the 64 bytes behind the capacity stay
    hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)
    torch.cuda.synchronize()
    assert torch.equal(st.masks, want) and bool((st.masks[16 * total:] == POISON).all())


@pytest.mark.parametrize("hw,canvas", [((24, 32), (96, 128)), ((25, 33), (150, 130)), ((40, 36), (160, 144))])
def test_borderline_pixels_take_the_post_processors_decision(hip, hw, canvas):
    """Per image at least 64 frame pixels whose float64 interpolant is below 2^-20 in magnitude (the construction of
    tests/test_eval_canvas_kernel_gpu.py): one fused multiply-add more or less flips several of them.  Every image has the canvas's
    size, and each original size samples every frame pixel: the identity, the exact double, and two generic up-scales."""
    (h, w), (Hc, Wc) = hw, canvas
    B, Q = 4, 2
    logits = torch.zeros(B, Q, h, w, dtype=torch.float64)
    for b in range(B):
        lg = _borderline_logits(h, w, Hc, Wc, seed=100 * h + b)
        near = int((np.abs(_bilinear64(lg, Hc, Wc)) < 2.0 ** -20).sum())
        assert near >= 64, (b, near)
        logits[b, 0] = torch.from_numpy(lg)
    logits[:, 1] = torch.randn(B, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h))
    dev = logits.float().contiguous().cuda()
    assert torch.equal(dev[:, 0].double().cpu(), logits[:, 0])                         # the solved logits are fp32 values
    sizes, origs = [canvas] * B, [canvas, (2 * Hc, 2 * Wc), (Hc + 7, Wc + 5), (2 * Hc + 1, 3 * Wc)]
    pred, valid = boxes_and_valid(B, 3, 1, [(0,), (1,), (2,), ()], h)
    total = hip.predict_layout(Q, origs)[-1]
    st = guarded_state(hip, B, 3, 16 * total)
    hip.predict_facts(sizes, origs, canvas, st.facts, Q=Q, capacity=st.capacity)
    before = st.masks.clone()
    hip.predict_canvas(pred, valid, st, pred_masks=dev, canvas_hw=canvas)
    torch.cuda.synchronize()
    want, _ = expected_buffer(hip, before, dev, sizes, origs, canvas)
    assert torch.equal(st.masks, want)


@pytest.mark.parametrize("P,K,valid_rows", [(3, 2, [(0, 1, 2), (), (1,), (0, 2)]),
                                            (70, 1, [tuple(range(70)), (), (62, 65, 69), (0, 10, 63, 64, 68)])])
def test_boxes_counts_and_unused_rows(hip, P, K, valid_rows):
    """P = 3 and P = 70 (the second 64-phrase pass); images with every phrase valid, with none, and with valid phrases on both sides of
    the pass boundary.  The rows start from poison: unused ones must come out 0."""
    B, origs = 4, [(333, 500), (1, 17), (96, 128), (480, 640)]
    pred, valid = boxes_and_valid(B, P, K, valid_rows, 100 + P)
    st = hip.PredictState(B, P, "cuda")
    st.block.fill_(POISON)
    hip.predict_facts([(24, 32)] * B, origs, (96, 128), st.facts)
    hip.predict_canvas(pred, valid, st)                                                # no masks: the box launch alone
    torch.cuda.synchronize()
    check_boxes(hip, st, pred, valid, origs)
    assert st.out_counts.tolist() == [len(r) for r in valid_rows]
    for b, rows in enumerate(valid_rows):
        assert bool((st.out_boxes[b, len(rows):] == 0).all())
        if rows:
            assert bool((st.out_boxes[b, :len(rows)] != 0).any())
    assert st.facts[:, 4:].cpu().tolist() == [[0, 0, 0, 0]] * B                        # Q = 0: no mask bytes


def test_replay_of_one_graph_reads_the_facts_on_the_device(hip):
    """rt_predict_canvas captured ONCE, replayed three times; between replays only rt_predict_facts is issued (other sizes, other
    originals) and the model-side tensors are overwritten in place.  Each replay equals its own oracle."""
    canvas, Q, B, P = (96, 128), 2, 3, 3
    batches = [([(75, 100), (96, 128), (48, 64)], [(150, 200), (37, 51), (96, 128)], [(0,), (1, 2), ()]),
               ([(24, 32), (60, 80), (96, 100)], [(1, 17), (60, 80), (201, 97)], [(0, 1, 2), (), (2,)]),
               ([(96, 128), (30, 41), (75, 100)], [(96, 128), (333, 500), (75, 100)], [(1,), (0,), (0, 2)])]
    cap = max(16 * hip.predict_layout(Q, o)[-1] for _, o, _ in batches) + 64
    st = guarded_state(hip, B, P, cap)
    logits = torch.zeros(B, Q, 24, 32, device="cuda")
    pred, valid = boxes_and_valid(B, P, 2, [(), (), ()], 0)
    hip.predict_facts(*batches[0][:2], canvas, st.facts, Q=Q, capacity=st.capacity)
    hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)          # (warm, uncaptured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)
    g = torch.Generator().manual_seed(31)
    for j, (sizes, origs, rows) in enumerate(batches):
        lg = torch.randn(B, Q, 24, 32, generator=g).cuda()
        pb, vb = boxes_and_valid(B, P, 2, rows, 40 + j)
        logits.copy_(lg); pred.copy_(pb); valid.copy_(vb)
        hip.predict_facts(sizes, origs, canvas, st.facts, Q=Q, capacity=st.capacity)
        torch.cuda.synchronize()
        before = st.masks.clone()
        graph.replay()
        torch.cuda.synchronize()
        want, off = expected_buffer(hip, before, lg, sizes, origs, canvas)
        assert torch.equal(st.masks, want), j
        assert torch.equal(st.masks[16 * off[-1]:], before[16 * off[-1]:]), j
        check_boxes(hip, st, pb, vb, origs)


@pytest.mark.parametrize("B", [1, 64])
def test_one_image_and_the_largest_batch(hip, B):
    assert B <= hip.BATCH_STAGE_MAX_B
    canvas, Q = (32, 48), 1
    g = torch.Generator().manual_seed(B)
    sizes = [(int(a), int(b)) for a, b in zip(torch.randint(1, 33, (B,), generator=g), torch.randint(1, 49, (B,), generator=g))]
    origs = [(int(a), int(b)) for a, b in torch.randint(1, 70, (B, 2), generator=g)]
    logits = torch.randn(B, Q, 8, 12, generator=g).cuda()
    pred, valid = boxes_and_valid(B, 5, 1, [tuple(range(b % 6)) for b in range(B)], B)
    total = hip.predict_layout(Q, origs)[-1]
    st = guarded_state(hip, B, 5, 16 * total)
    hip.predict_facts(sizes, origs, canvas, st.facts, Q=Q, capacity=st.capacity)
    before = st.masks.clone()
    hip.predict_canvas(pred, valid, st, pred_masks=logits, canvas_hw=canvas)
    torch.cuda.synchronize()
    want, off = expected_buffer(hip, before, logits, sizes, origs, canvas)
    assert torch.equal(st.masks, want)
    assert st.facts[:, 4].cpu().tolist() == off[:-1] and int(st.facts[B - 1, 5]) == total
    check_boxes(hip, st, pred, valid, origs)


def test_argument_checks_leave_the_outputs_alone(hip):
    canvas, Q, B, P = (96, 128), 2, 2, 3
    logits = torch.randn(B, Q, 24, 32).cuda()
    pred, valid = boxes_and_valid(B, P, 2, [(0,), (1,)], 1)
    st = guarded_state(hip, B, P, 1 << 16, behind=0)
    st.facts.fill_(-7)
    stream = torch.cuda.current_stream().cuda_stream
    L, n = hip.lib(), hip.BATCH_STAGE_MAX_B
    arr = lambda v: (ctypes.c_int32 * n)(*v)

    def facts(**kw):
        f = dict(facts=st.facts.data_ptr(), capacity=st.capacity, B=B, Q=Q, Hc=96, Wc=128, img_h=arr([75, 96]), img_w=arr([100, 128]),
                 orig_h=arr([75, 37]), orig_w=arr([100, 51]))
        f.update(kw)
        return L.rt_predict_facts(ctypes.byref(hip.PredictFactsArgs(**f)), stream)
    BAD, UNSUPPORTED = -1, -2
    assert L.rt_predict_facts(None, stream) == BAD
    for kw in (dict(facts=None), dict(B=0), dict(B=-1), dict(Q=-1), dict(capacity=-1), dict(Hc=0), dict(Wc=0),
               dict(img_h=arr([0, 96])), dict(img_w=arr([100, -3])), dict(orig_h=arr([75, 0])), dict(orig_w=arr([0, 51])),
               dict(img_h=arr([97, 96])), dict(img_w=arr([100, 129])),                 # larger than the canvas
               dict(capacity=16 * hip.predict_layout(Q, [(75, 100), (37, 51)])[-1] - 16)):   # one unit short
        assert facts(**kw) == BAD, kw
    assert facts(B=n + 1) == UNSUPPORTED
    assert facts(capacity=1 << 40, orig_h=arr([32768, 37]), orig_w=arr([32768, 51])) == UNSUPPORTED          # 2 * 2^30 bytes >= 2^31
    assert facts(capacity=16 * hip.predict_layout(Q, [(75, 100), (37, 51)])[-1]) == 0                        # exactly enough (launched)
    torch.cuda.synchronize()
    assert st.facts[:, :4].cpu().tolist() == [[75, 100, 75, 100], [96, 128, 37, 51]]
    st.facts.fill_(-7)
    st.block.fill_(POISON)

    def run(**kw):
        f = dict(pred_boxes=pred.data_ptr(), valid=valid.data_ptr(), facts=st.facts.data_ptr(), pred_masks=logits.data_ptr(),
                 out_boxes=st.out_boxes.data_ptr(), out_counts=st.out_counts.data_ptr(), out_masks=st.masks.data_ptr(),
                 capacity=st.capacity, B=B, P=P, K=2, Q=Q, h=24, w=32, Hc=96, Wc=128, threshold=0.5)
        f.update(kw)
        return L.rt_predict_canvas(ctypes.byref(hip.PredictCanvasArgs(**f)), stream)
    assert L.rt_predict_canvas(None, stream) == BAD
    for name in ("pred_boxes", "valid", "facts", "out_boxes", "out_counts", "out_masks"):
        assert run(**{name: None}) == BAD, name
    for name in ("B", "P", "K", "Q", "h", "w", "Hc", "Wc"):
        assert run(**{name: 0}) == BAD, name
    assert run(capacity=-16) == BAD
    for shift in (1, 4, 8):
        assert run(out_masks=st.masks.data_ptr() + shift) == BAD, shift               # not 16-byte aligned
    assert run(B=n + 1) == UNSUPPORTED and run(capacity=1 << 31) == UNSUPPORTED
    assert run(Hc=1 << 16, Wc=1 << 15) == UNSUPPORTED and run(h=1 << 16, w=1 << 15) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((st.block == POISON).all()) and bool((st.facts == -7).all())           # nothing was launched
