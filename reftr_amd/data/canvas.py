"""The batch canvas: one fixed input shape for data whose batches all differ.

The reference's collate (util/collate_fn.py:24-41) pads a batch to the largest image IN that batch, Flickr30k Entities carries a
different number of boxes per image, RES target masks have the size of their image -- so nearly every batch has its own shape, and a
step captured into a hipGraph for one shape (engine_vg.CapturedTrainStep) serves almost none of them.  A BatchCanvas fixes the shape:
images are padded to (height, width) with zeros on the right and bottom, the padding mask with True, the target masks with zeros,
and the target boxes are packed into a buffer of `boxes_per_image` rows per image with their offsets and their count kept in device
memory.  That is the batch the reference's collate produces whenever one image of the batch has the canvas size, so the step computed
on it is the existing code's step at an existing shape.

`pad_on_host` is that definition in plain torch; `stage` is the same bytes written by ONE rt_batch_stage launch into buffers that
stay where they are, which is what a captured step needs.  Opt-in: engine_vg's entry points take `canvas=None`.

A RAW batch (reftr_amd.data.raw: `samples["img"]` a RawImages, targets in the raw frame) is defined the same way: `pad_on_host` runs
the DeviceInputPipeline chain to the canvas's size and then the padding above; `stage` writes the same bytes with ONE rt_raw_stage
launch -- resize, ToTensor, Normalize, the target transforms and the padding all happen on the way into the buffers.  A raw batch
that carries gains (RawImages.gains: the reference's RandomIntensitySaturation, reftr_amd.data.jitter) is colour-jittered first, on
both paths, by one rt_hsv_jitter launch into a scratch; a batch without gains issues the launches it always did.
"""
import torch

from .. import hip as H
from ..util.misc import NestedTensor
from .device_input import MEAN, STD, DeviceInputPipeline
from .raw import RawImages


def _token_shapes(samples):
    """The fields a canvas leaves alone (sentence, phrase, their masks and positions ...): name -> shape without the batch axis."""
    return tuple((k, tuple(v.shape[1:])) for k, v in sorted(samples.items()) if torch.is_tensor(v))


class StagedBatch:
    """The static buffers of one canvas batch: `samples` (the canvas-sized 'img' NestedTensor + the token fields), `targets_static`
    = (boxes [B * boxes_per_image, 4] fp32, tgt_off [B + 1] int32, num_boxes [1] fp32) and `tgt_masks` (uint8 [B, 1, H, W] or None).
    `jitter_scratch`: the uint8 bytes rt_hsv_jitter writes and rt_raw_stage reads when a raw batch carries gains (None until one
    does; it grows when a batch needs more)."""

    def __init__(self, samples, targets_static, tgt_masks):
        self.samples, self.targets_static, self.tgt_masks = samples, targets_static, tgt_masks
        self.jitter_scratch = None


class BatchCanvas:
    """One fixed input shape: (height, width) images, `boxes_per_image` box rows per image, target masks when `masks`.

    A canvas EVALUATION batch (engine_vg.evaluate(canvas=...)) is the batch the reference's collate and evaluation loop would
    produce if the batch held one canvas-sized image:
      * forward and losses run on pad_on_host(samples, targets): image zero-padded to the canvas, padding mask True outside, target
        masks zero-padded to the canvas;
      * the mask post-processor's padded frame IS the canvas: `pred_masks` covers the canvas, so the logits are resized to
        (height, width) -- in the reference the frame is the largest `size` of the batch, which is the same number there because the
        batch is padded to its largest image -- and each image is then cropped to its own `size`;
      * box metrics, the results' boxes (scaled to `orig_size`) and the mask {I, U} are what the existing kernels give on that frame
        with the un-padded targets.
    Nothing about a batch that already has the canvas's size changes."""

    def __init__(self, height, width, boxes_per_image, masks=False, tokens=None):
        self.height, self.width, self.boxes_per_image, self.masks = int(height), int(width), int(boxes_per_image), bool(masks)
        assert self.height > 0 and self.width > 0 and self.boxes_per_image > 0
        self.tokens = tokens                     # token field shapes, bound by the first batch (from_args / bind)
        self._pipes = {}                         # (size, max_size, padded to the canvas) -> the DeviceInputPipeline of a raw batch

    @classmethod
    def from_args(cls, args, samples, masks=None):
        """The canvas of a run: `max_img_size` squared (what datasets/transforms.py:84-102 can produce at most), as many boxes per
        image as the batch has phrase slots (1 without a phrase field), target masks when the run trains the segmentation head."""
        size = int(args.max_img_size)
        cap = int(samples["phrase"].shape[1]) if "phrase" in samples else 1
        if masks is None:
            masks = bool(getattr(args, "masks", False))
        return cls(size, size, cap, masks=masks).bind(samples)

    def bind(self, samples):
        """Fixes the token field shapes to those of `samples` (the datasets pad them to a fixed length)."""
        self.tokens = _token_shapes(samples)
        return self

    def __repr__(self):
        return f"BatchCanvas({self.height}, {self.width}, boxes_per_image={self.boxes_per_image}, masks={self.masks})"

    def key(self, samples):
        """What a capture on this canvas depends on: the canvas, the batch size and the token field shapes -- not the image size, not
        the box counts, not the target mask sizes."""
        img = samples["img"]
        B = len(img) if isinstance(img, RawImages) else int(img.tensors.shape[0])
        return ("canvas", self.height, self.width, self.boxes_per_image, self.masks, B, _token_shapes(samples))

    def _why_not_raw(self, img, targets):
        """The image and mask part of why_not for a raw batch."""
        if not img.well_formed():
            if img.gains is not None and RawImages(img.images, img.size, img.max_size).well_formed():
                return "gains that are not one finite, non-negative (s_gain, v_gain) pair per image"
            return "a raw image that is not uint8 [h, w, 3]"
        S = H.RAW_STAGE_MAX_SCALE
        for im, (oh, ow) in zip(img.images, img.out_sizes()):
            h, w = int(im.shape[0]), int(im.shape[1])
            if oh <= 0 or ow <= 0 or oh > self.height or ow > self.width:
                return f"raw image {h} x {w} resized to {oh} x {ow} exceeds the canvas"
            if h > S * oh or w > S * ow:
                return f"raw image {h} x {w} resized to {oh} x {ow} is scaled down by more than {S}"
        if self.masks and len(targets) == len(img):
            for im, t in zip(img.images, targets):
                m = t.get("masks")
                if m is not None and m.dim() == 3 and tuple(m.shape[-2:]) != tuple(im.shape[:2]):
                    return f"target mask {m.shape[-2]} x {m.shape[-1]} on a raw image {im.shape[0]} x {im.shape[1]}"
        return None

    def why_not(self, samples, targets):
        """None when the batch fits, else the reason as a short phrase."""
        img = samples.get("img")
        if isinstance(img, RawImages):
            why = self._why_not_raw(img, targets)
            return why if why is not None else self._why_not_rest(samples, targets, len(img), raw=True)
        if not isinstance(img, NestedTensor) or img.tensors.dim() != 4 or img.tensors.shape[1] != 3:
            return "no [B, 3, h, w] image NestedTensor"
        B, _, h, w = img.tensors.shape
        if h > self.height or w > self.width:
            return f"image {h} x {w} exceeds the canvas"
        return self._why_not_rest(samples, targets, B)

    def _why_not_rest(self, samples, targets, B, raw=False):
        """Batch size, token fields, boxes and target masks: the same for both forms of a batch (a raw mask has its image's size and is
        resized with it, so it cannot exceed the canvas)."""
        if B > H.BATCH_STAGE_MAX_B:
            return f"more than {H.BATCH_STAGE_MAX_B} images"
        if len(targets) != B:
            return "targets do not match the batch"
        if self.tokens is not None and _token_shapes(samples) != self.tokens:
            return "token field shapes differ from the canvas's"
        for t in targets:
            n = int(t["boxes"].shape[0])
            if "labels" in t and len(t["labels"]) != n:
                # the existing criterion counts len(labels) into num_boxes, the staged count is the number of box rows: a canvas step is
                # the existing step only where the two agree (they do in every dataset of the reference)
                return f"{len(t['labels'])} labels for {n} boxes on an image"
            if n > self.boxes_per_image:
                return f"{n} boxes on an image, capacity {self.boxes_per_image}"
            if self.masks:
                m = t.get("masks")
                if m is None or m.dim() != 3 or m.shape[0] != 1:
                    return "no [1, h, w] target mask"
                if not raw and (m.shape[-2] > self.height or m.shape[-1] > self.width):
                    return f"target mask {m.shape[-2]} x {m.shape[-1]} exceeds the canvas"
        return None

    def fits(self, samples, targets):
        return self.why_not(samples, targets) is None

    def why_not_eval(self, samples, targets, segm=False):
        """What engine_vg.evaluate(canvas=...) asks of a batch ON TOP of why_not: None, or the reason as a short phrase.  The metric
        tail of a canvas evaluation reads every per-image fact from device memory (rt_eval_facts gathers them), so every target must
        carry them in the one form the gather takes: `size` as an int64 pair, `orig_size` likewise when any target has it, `image_id`
        (one int64) on all targets or on none, and -- with a 'segm' post-processor -- a one-byte [1, h, w] target mask on a masks=True
        canvas.  Tensor shapes, dtypes and key presence only: nothing is read from the device."""
        def pair(v, n):
            return torch.is_tensor(v) and v.dtype == torch.int64 and v.numel() == n
        if segm and not self.masks:
            return "a 'segm' post-processor needs a masks=True canvas"
        any_orig = any("orig_size" in t for t in targets)
        with_id = sum(1 for t in targets if "image_id" in t)
        if with_id not in (0, len(targets)):
            return "image_id on some targets only"
        for t in targets:
            if not pair(t.get("size"), 2):
                return "no int64 [2] size on a target"
            if any_orig and not pair(t.get("orig_size"), 2):
                return "no int64 [2] orig_size on a target while another has one"
            if with_id and not pair(t["image_id"], 1):
                return "an image_id that is not one int64"
            if segm:
                m = t.get("masks")
                if m is None or m.dim() != 3 or m.shape[0] != 1 or m.element_size() != 1:
                    return "no one-byte [1, h, w] target mask"
        return None

    def why_not_eval_raw(self, samples, targets, segm=False):
        """What engine_vg.evaluate_raw asks of a RAW batch on top of why_not: None, or the reason as a short phrase.  `size` and
        `orig_size` are not asked of the targets -- they are RawImages.out_sizes() and the raw images' own (h, w), host values that reach
        the device by value (rt_eval_raw_facts).  `image_id` (one int64) is on all targets or on none; with a 'segm' post-processor the
        canvas has masks=True and every target a one-byte [1, h, w] mask of its image's size: rt_eval_orig reads it where it lies.
        Shapes, dtypes and key presence only: nothing is read from the device."""
        img = samples.get("img")
        if segm and not self.masks:
            return "a 'segm' post-processor needs a masks=True canvas"
        with_id = sum(1 for t in targets if "image_id" in t)
        if with_id not in (0, len(targets)):
            return "image_id on some targets only"
        for im, t in zip(img.images, targets):
            v = t.get("image_id")
            if with_id and not (torch.is_tensor(v) and v.dtype == torch.int64 and v.numel() == 1):
                return "an image_id that is not one int64"
            if segm:
                m = t.get("masks")
                if m is None or m.dim() != 3 or m.shape[0] != 1 or m.element_size() != 1:
                    return "no one-byte [1, h, w] target mask"
                if tuple(m.shape[-2:]) != tuple(im.shape[:2]):
                    return f"target mask {m.shape[-2]} x {m.shape[-1]} on a raw image {im.shape[0]} x {im.shape[1]}"
        return None

    def raw_targets(self, samples, targets):
        """The plain-torch restatement of what evaluate_raw knows about a raw batch without reading its targets: `targets` with `size`
        (RawImages.out_sizes()) and `orig_size` (the raw (h, w)) added as int64 pairs on the images' device -- what a loader of the
        NestedTensor form would have collated.  `image_id` stays as it is."""
        img = samples["img"]
        out = []
        for im, (oh, ow), t in zip(img.images, img.out_sizes(), targets):
            t = dict(t)
            t["size"] = torch.tensor([oh, ow], dtype=torch.int64, device=im.device)
            t["orig_size"] = torch.tensor([int(im.shape[0]), int(im.shape[1])], dtype=torch.int64, device=im.device)
            out.append(t)
        return out

    def resized_eval(self, samples, targets):
        """What a raw evaluation batch MEANS for the existing keys, in plain torch: `resized` (the DeviceInputPipeline chain) with
        `size`, `orig_size` and `image_id` added as tensors -- the batch evaluate(canvas=) takes."""
        s, t = self.resized(samples, targets)
        for new, facts in zip(t, self.raw_targets(samples, targets)):
            new["size"], new["orig_size"] = facts["size"], facts["orig_size"]
            if "image_id" in facts:
                new["image_id"] = facts["image_id"]
        return s, t

    # ------------------------------------------------------------------ the definition, in plain torch
    def resized(self, samples, targets, to_canvas=False):
        """A raw batch through the existing device chain (DeviceInputPipeline: rt_resample_u8 per pass and image, rt_img_collate_norm,
        the target transforms in torch): the NestedTensor form of the batch, collated to its own largest image -- or, `to_canvas`,
        straight to the canvas's size.  A batch that carries gains is jittered in front of the chain by rt_hsv_jitter, whose bytes are
        reftr_amd.data.jitter.apply's."""
        img = samples["img"]
        pkey = (img.size, img.max_size, bool(to_canvas))
        if pkey not in self._pipes:
            self._pipes[pkey] = DeviceInputPipeline(img.size, img.max_size, device=img.device if img.is_cuda else "cuda",
                                                    pad_to=(self.height, self.width) if to_canvas else None)
        images = img.images
        if img.gains is not None:                # the colour jitter first, on the raw bytes, into temporaries (rt_hsv_jitter)
            images = self._jittered(img if img.is_cuda else img.to(self._pipes[pkey].device, non_blocking=True))
        nested, out_t = self._pipes[pkey](images, targets)
        s = dict(samples)
        s["img"] = nested
        return s, out_t

    def pad_on_host(self, samples, targets):
        """The batch as the reference's collate would deliver it with one canvas-sized image in it: new tensors, any device.  A raw
        batch: what the existing device chain makes of it (`resized`), padded the same way."""
        assert self.fits(samples, targets), self.why_not(samples, targets)
        if isinstance(samples["img"], RawImages):
            samples, targets = self.resized(samples, targets, to_canvas=True)
        img = samples["img"]
        B, C, h, w = img.tensors.shape
        t = img.tensors.new_zeros((B, C, self.height, self.width))
        t[:, :, :h, :w] = img.tensors
        m = torch.ones((B, self.height, self.width), dtype=torch.bool, device=img.mask.device)
        m[:, :h, :w] = img.mask
        s = dict(samples)
        s["img"] = NestedTensor(t, m)
        out_t = []
        for tg in targets:
            tg = dict(tg)
            if self.masks:
                src = tg["masks"]
                pm = src.new_zeros((src.shape[0], self.height, self.width))
                pm[:, :src.shape[-2], :src.shape[-1]] = src
                tg["masks"] = pm
            out_t.append(tg)
        return s, out_t

    # ------------------------------------------------------------------ the same bytes from one launch
    def alloc(self, samples):
        """Static buffers for batches like `samples` (B, token shapes, device); the token fields start as copies of `samples`'s."""
        img = samples["img"]
        dev, B = (img.device, len(img)) if isinstance(img, RawImages) else (img.tensors.device, int(img.tensors.shape[0]))
        s = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in samples.items() if k != "img"}
        s["img"] = NestedTensor(torch.empty((B, 3, self.height, self.width), dtype=torch.float32, device=dev),
                                torch.empty((B, self.height, self.width), dtype=torch.bool, device=dev))
        static = (torch.empty((B * self.boxes_per_image, 4), dtype=torch.float32, device=dev),
                  torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.float32, device=dev))
        tm = torch.empty((B, 1, self.height, self.width), dtype=torch.uint8, device=dev) if self.masks else None
        return StagedBatch(s, static, tm)

    def stage(self, samples, targets, out=None, tokens=True):
        """Writes the batch into `out` (a StagedBatch; a fresh one when None) with one launch on the current stream -- rt_batch_stage,
        or rt_raw_stage for a raw batch -- and returns it.  `tokens=False` leaves the token fields to the caller (the engine copies
        them with its grouped copy)."""
        assert self.fits(samples, targets), self.why_not(samples, targets)
        fresh = out is None
        if fresh:
            out = self.alloc(samples)
        img = samples["img"]
        if isinstance(img, RawImages):
            self._stage_raw(img, targets, out)
        else:
            self._stage_nested(img, targets, out)
        if tokens and not fresh:
            for k, v in samples.items():
                if torch.is_tensor(v):
                    out.samples[k].copy_(v, non_blocking=True)
        return out

    @staticmethod
    def _boxes(targets):
        """The boxes of `targets` as the stage calls take them: fp32, contiguous."""
        return [(t["boxes"] if t["boxes"].dtype == torch.float32 else t["boxes"].float()).contiguous() for t in targets]

    def _masks(self, targets, raw):
        """The target masks as one-byte contiguous tensors, None without masks.  What is not a byte already is converted as its form of
        batch defines, and the two differ in meaning: a raw mask is resized with its image and DeviceInputPipeline._target thresholds it,
        `.float() > 0.5`; the mask of a NestedTensor batch is only padded and keeps its values, `.to(torch.uint8)`."""
        convert = (lambda m: m.float() > 0.5) if raw else (lambda m: m.to(torch.uint8))
        return [(t["masks"] if t["masks"].element_size() == 1 else convert(t["masks"])).contiguous() for t in targets] if self.masks else None

    @staticmethod
    def _jittered(img, holder=None):
        """The images the resize reads: a raw batch's own, contiguous -- or, when it carries gains, their colour-jittered copies
        (reftr_amd.data.jitter.apply's bytes) written by ONE rt_hsv_jitter launch on the current stream into a uint8 scratch, each image
        at a 16-byte aligned offset.  The scratch is `holder.jitter_scratch` (a StagedBatch's: kept, and replaced by a larger one when
        a batch needs more) or a temporary; it is allocated and used under the current stream.  The batch's tensors are never written."""
        images = [im.contiguous() for im in img.images]
        if img.gains is None:
            return images
        offsets, total = [], 0
        for im in images:
            offsets.append(total)
            total += -(-im.numel() // 16) * 16
        dev = images[0].device
        scratch = holder.jitter_scratch if holder is not None else None
        if scratch is None or scratch.numel() < total or scratch.device != dev:
            scratch = torch.empty(total, dtype=torch.uint8, device=dev)
            if holder is not None:
                holder.jitter_scratch = scratch
        else:
            scratch.record_stream(torch.cuda.current_stream(dev))          # (kept from an earlier call: perhaps under another stream)
        outs = [scratch[o:o + im.numel()].view(im.shape) for o, im in zip(offsets, images)]
        H.hsv_jitter(images, img.gains, outs)
        return outs

    def _stage_raw(self, img, targets, out):
        H.raw_stage(self._jittered(img, out), img.out_sizes(), out.samples["img"].tensors, out.samples["img"].mask,
                    self._boxes(targets), self.boxes_per_image, *out.targets_static, MEAN, STD, mask_list=self._masks(targets, True),
                    tgt_masks=out.tgt_masks)

    def _stage_nested(self, img, targets, out):
        src = img.tensors if img.tensors.dtype == torch.float32 else img.tensors.float()
        src_mask = img.mask if img.mask.element_size() == 1 else img.mask.bool()
        H.batch_stage(src.contiguous(), src_mask.contiguous(), out.samples["img"].tensors, out.samples["img"].mask, self._boxes(targets),
                      self.boxes_per_image, *out.targets_static, mask_list=self._masks(targets, False), tgt_masks=out.tgt_masks)
