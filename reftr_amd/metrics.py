"""Evaluation metrics of engine_vg.evaluate on the device (csrc/rt_eval.hip, ABI rt_eval_metrics).

One call per batch scores every valid phrase's box against its target box and, for a RES model, query 0's post-processed mask
against the target mask; the running totals (counts int64, IoU sums double) stay in a 16-slot device tensor that is read back ONCE
per evaluation.  On top of the reference's Acc@0.5 / mean IoU / mean mask IoU (engine_vg.py:127-152, 205-219) the totals carry what
every referring-segmentation table reports: overall IoU (total intersection over total union) and Pr@0.5 ... 0.9.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import hip as H
from .util import misc as utils

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


def build_table(targets, sizes=None):
    """The host side of rt_eval_metrics' per-image table, from tensor SHAPES only (nothing is read from the device).
    targets: the evaluation loop's list of dicts ('boxes' fp32 [n_b, 4] cxcywh; 'masks' [h, w] or [1, h, w], bool or uint8, when
    `sizes` is given).  sizes: per image (img_h, img_w) python ints, the post-processor's crop; a target mask of another size raises the
    reference's assertion (util/box_ops.py mask_iou).
    Returns (words, keep): words = int64 CPU tensor, B rows of {boxes pointer, n_b, mask pointer | 0, mask h, mask w}, followed -- when
    `sizes` is given -- by B words that each hold one image's {img_h, img_w} as two int32 (the kernel's `sizes` argument, so table and
    sizes travel in ONE copy); keep = the tensors whose pointers the table names (contiguous copies where the input was not): the
    caller holds them until the kernel has run."""
    rows, keep = [], []
    for b, tg in enumerate(targets):
        boxes = tg["boxes"]
        if boxes.dtype != torch.float32 or not boxes.is_contiguous():
            boxes = boxes.to(torch.float32).contiguous()
        assert boxes.dim() == 2 and boxes.shape[1] == 4, boxes.shape
        keep.append(boxes)
        mp = mh = mw = 0
        if sizes is not None:
            m = tg["masks"]
            if m.dim() == 3:
                assert m.shape[0] == 1, m.shape
                m = m[0]
            assert m.dim() == 2, m.shape
            assert tuple(m.shape[-2:]) == (int(sizes[b][0]), int(sizes[b][1])), (tuple(m.shape), tuple(sizes[b]))
            if m.dtype not in (torch.bool, torch.uint8):
                m = m != 0
            m = m.contiguous()
            keep.append(m)
            mp, (mh, mw) = m.data_ptr(), m.shape
        rows.append([boxes.data_ptr(), boxes.shape[0], mp, mh, mw])
    words = [v for r in rows for v in r]
    if sizes is not None:
        words += [int(s[0]) | (int(s[1]) << 32) for s in sizes]
    return torch.tensor(words, dtype=torch.int64), keep


def stats_from_accumulators(slots, seg=False, world=1, local_seg_n=0):
    """The evaluation statistics from the RT_EVAL_SLOTS accumulator values (python ints, the two sums python floats), already summed
    over the ranks.  Pure host arithmetic.  'accuracy_iou0.5' and 'miou' divide by the pair count clamped to 1 as the reference's
    cnt.clamp(min=1); 'seg_miou' is the reference's formula, sum / (world x this rank's sample count) (engine_vg.py:212-219); the
    keys the reference does not have -- 'seg_oiou' and 'seg_prec@t' -- use the summed counts."""
    det_n = max(int(slots[H.EVAL_DET_N]), 1)
    stats = {"accuracy_iou0.5": float(np.float32(slots[H.EVAL_DET_HIT]) / np.float32(det_n)),     # fp32 quotient, as before
             "miou": float(slots[H.EVAL_DET_SUM]) / det_n}
    if seg:
        stats["seg_miou"] = float(slots[H.EVAL_SEG_SUM]) / max(float(world * local_seg_n), 1.0)
        union = int(slots[H.EVAL_SEG_U])
        stats["seg_oiou"] = int(slots[H.EVAL_SEG_I]) / union if union else float("nan")
        seg_n = max(int(slots[H.EVAL_SEG_N]), 1)
        for t, thr in enumerate(THRESHOLDS):
            stats[f"seg_prec@{thr}"] = int(slots[H.EVAL_SEG_HIT + t]) / seg_n
    return stats


def stats_from_orig_accumulators(slots):
    """The original-frame mask statistics from the RT_EVAL_ORIG_SLOTS accumulator values (python ints, the sum a python float), summed
    over the ranks: stats_from_accumulators' mask formulas applied to counts taken on the raw frame against the raw annotation
    (rt_eval_orig).  'seg_miou_orig' = the double sum of the fp32 IoUs / the sample count, 'seg_oiou_orig' = total intersection /
    total union (NaN without a union), 'seg_prec@t_orig' = hits / the sample count; the count is clamped to 1.  Pure host arithmetic."""
    n = max(int(slots[H.EVAL_ORIG_N]), 1)
    union = int(slots[H.EVAL_ORIG_U])
    stats = {"seg_miou_orig": float(slots[H.EVAL_ORIG_SUM]) / n,
             "seg_oiou_orig": int(slots[H.EVAL_ORIG_I]) / union if union else float("nan")}
    for t, thr in enumerate(THRESHOLDS):
        stats[f"seg_prec@{thr}_orig"] = int(slots[H.EVAL_ORIG_HIT + t]) / n
    return stats


def decode_ring(boxes, counts, ids, cursor, overflow, batches):
    """The results ring of rt_eval_canvas, read back once after an evaluation, as one results dict per slot (the caller merges them
    in loader order).  Pure host work on numpy arrays:
    boxes float32 [slots, B, P, 4], counts int32 [slots, B], ids int64 [slots, B]; cursor / overflow: the two device words as ints;
    batches: one (batch number in the loader, has_ids, [target boxes per image as the host knew them from shapes]) per slot, in
    the order the batches were replayed.
    dict[int(image_id)] = the image's boxes as nested lists of python floats (float64 holds every fp32 coordinate exactly;
    the ids stay integers).  An image of a batch without `image_id` is skipped.  The reference's assertion -- as many result boxes
    as target boxes, engine_vg.py:128 -- is checked here, naming the batch and the image.  A ring that overflowed, or whose cursor
    is not the number of replayed batches, raises RuntimeError: results would be missing."""
    if overflow:
        raise RuntimeError(f"evaluation results ring overflowed ({boxes.shape[0]} slots, {len(batches)} batches replayed)")
    if int(cursor) != len(batches):
        raise RuntimeError(f"evaluation results ring holds {int(cursor)} batches, {len(batches)} were replayed")
    out = []
    for slot, (number, has_ids, n_boxes) in enumerate(batches):
        out.append({})
        for b, n in enumerate(n_boxes):
            c = int(counts[slot, b])
            assert c == int(n), f"batch {number}, image {b}: {c} result boxes for {int(n)} target boxes"
            if has_ids:
                out[-1][int(ids[slot, b])] = np.asarray(boxes[slot, b, :c], dtype=np.float64).tolist()
    return out


class EvalMeter:
    """Running evaluation metrics on `device`: update() per batch (two kernel launches, one host-to-device copy, no sync),
    compute() once at the end (one all-reduce pair under torch.distributed, one device-to-host copy)."""

    def __init__(self, device, seg=None):
        """seg: whether compute() reports the mask keys; None: iff an update scored masks."""
        self.device = torch.device(device)
        self._seg = seg
        # one block, so that both sets of totals are zeroed by one launch and leave in one copy: `acc` (rt_eval_metrics /
        # rt_eval_canvas) and behind it `acc_orig`, the original-frame mask totals of a raw evaluation (rt_eval_orig)
        self._block = torch.zeros(H.EVAL_SLOTS + H.EVAL_ORIG_SLOTS, dtype=torch.int64, device=self.device)
        self.acc, self.acc_orig = self._block[:H.EVAL_SLOTS], self._block[H.EVAL_SLOTS:]
        self.reset()

    def reset(self, fresh=True):
        """Zeroes the accumulators now.  fresh: the next update also starts them from zero inside its own launch; False for a loop in
        which another producer (engine_vg.CapturedEvalStep: rt_eval_canvas inside a replayed graph) adds to `acc` beside update()."""
        self._block.zero_()
        self._fresh = fresh
        self.seg = bool(self._seg)
        self.orig = False
        self.local_seg_n = 0
        self.last = None
        self._keep = None

    def book(self, n_images, seg):
        """Books a batch that was added to `acc`, by update() or by the other producer: the mask keys and this rank's seg sample count."""
        if seg:
            self.seg = True if self._seg is None else self.seg
            self.local_seg_n += int(n_images)

    def book_orig(self):
        """Books that a producer adds to `acc_orig`: compute() reports the '_orig' keys."""
        self.orig = True

    @torch.no_grad()
    def update(self, outputs, targets, masks=None, sizes=None):
        """outputs: the model's dict ('pred_boxes' [B, P, K, 4], 'phrase_mask' [B, P(*K)]); targets: list of dicts with 'boxes' (and
        'masks' when `masks` is given); masks: uint8 / bool [B, Q, max_h, max_w], the frame hip.mask_postprocess wrote; sizes: per image
        (img_h, img_w) as python ints.  Launches on torch's current stream."""
        boxes = outputs["pred_boxes"]
        B, P, K, _ = boxes.shape
        assert B == len(targets)
        boxes = boxes.to(torch.float32).contiguous()
        valid = outputs["phrase_mask"].reshape(B, P, K).to(torch.uint8).contiguous()
        if masks is not None:
            assert sizes is not None and len(sizes) == B
            masks = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()
        words, keep = build_table(targets, sizes if masks is not None else None)
        dev = words.to(boxes.device)                                         # the ONE host-to-device copy
        table = dev[:5 * B].view(B, 5)
        sizes_dev = dev[5 * B:].view(torch.int32).view(B, 2) if masks is not None else None
        iou_det, iou_seg, iu = H.eval_metrics(boxes, valid, table, self.acc, masks=masks, sizes_i32=sizes_dev, reset=self._fresh)
        self._fresh = False
        self.book(B, masks is not None)
        self._keep = (keep, dev, boxes, valid, masks)                        # alive until the next update
        self.last = SimpleNamespace(iou_det=iou_det, iou_seg=iou_seg, iu=iu)

    @torch.no_grad()
    def compute(self, world_reduce=True):
        block = self._block
        world = 1
        if world_reduce and utils.is_dist_avail_and_initialized():
            world = utils.get_world_size()
            block = block.clone()
            torch.distributed.all_reduce(block[:H.EVAL_DET_SUM])                                     # the int64 counts
            torch.distributed.all_reduce(block[H.EVAL_DET_SUM:H.EVAL_SLOTS].view(torch.float64))     # the two double sums
            # (acc_orig is not reduced: a raw evaluation runs on one rank)
        host = block.cpu()                                                   # the ONE device-to-host copy
        acc, orig = host[:H.EVAL_SLOTS], host[H.EVAL_SLOTS:]
        slots = acc[:H.EVAL_DET_SUM].tolist() + acc[H.EVAL_DET_SUM:].view(torch.float64).tolist()
        stats = stats_from_accumulators(slots, seg=self.seg, world=world, local_seg_n=self.local_seg_n)
        if self.orig:
            stats.update(stats_from_orig_accumulators(orig[:H.EVAL_ORIG_SUM].tolist() + orig[H.EVAL_ORIG_SUM:].view(torch.float64).tolist()))
        return stats
