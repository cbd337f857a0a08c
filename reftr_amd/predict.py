"""Prediction: raw images and phrases in, boxes in original pixels and -- for RES -- masks at the original resolution out.

    p = Predictor(model, postprocessors, canvas, max_orig_size=(H, W))
    results = p(samples)          # samples["img"]: a reftr_amd.data.RawImages (host or device), plus the token fields

WHAT A PREDICTION IS (the definition; tests/test_predict_gpu.py computes it from these public pieces):
  * the forward in eval mode on canvas.pad_on_host(samples, targets without boxes): the DeviceInputPipeline chain to the canvas's
    size, zero padded, as in canvas training and evaluation;
  * boxes:  hip.box_postprocess(pred_boxes, phrase_mask, sizes_f32 = the raw images' (h, w)) -- PostProcessVGMultiPhrase scaled to
    the original size;
  * masks (with a 'segm' post-processor): masks_origin of hip.mask_postprocess(pred_masks, sizes = RawImages.out_sizes(), max_hw =
    the canvas, orig = the raw images' (h, w)) at the post-processor's threshold -- PostProcessSegm with the canvas as its padded
    frame, exactly as in canvas evaluation.

Per batch the host issues rt_raw_stage (no boxes, no target masks), rt_predict_facts, the grouped copy of the token fields and ONE
replay of ONE graph per canvas key (forward -> rt_predict_canvas), then one device -> host copy into pinned memory whose size is known
from the shapes alone (the header and the used mask bytes are contiguous), and one wait.  Nothing is read from the device to decide
anything.  A batch that does not fit (why_not) runs through the existing chain at its own shape -- BatchCanvas.resized -> the model
-> the two post-processors -- with the same result structure; said once per reason on stderr.
"""
import torch

from . import hip as H
from .data.raw import RawImages
from .engine_vg import (_before_forward_replay, _canvas_single_process, _capture, _copy_batch, _inner, _run_again_on_chain, _say_once,
                        _state, _to_device, _warm_up)

mask_layout = H.predict_layout          # (Q, [(orig_h, orig_w)]) -> off16[0 .. B]: the packed mask blocks, in 16-byte units


def header_bytes(B, P):
    """Bytes of a result block's header: boxes fp32 [B, P, 4], counts int32 [B], rounded up to 16 (hip.PredictState's layout)."""
    return -(-(B * P * 16 + B * 4) // 16) * 16


def decode_block(block, B, P, origs, Q=0):
    """Per-image views of a packed result block (uint8, host): [{"boxes": fp32 [n_b, 4], "masks": uint8 [Q, 1, orig_h, orig_w]}]
    ("masks" only when Q > 0).  `origs`: the images' original (h, w).  Views, no copies."""
    nb = B * P * 16
    boxes = block[:nb].view(torch.float32).view(B, P, 4)
    counts = block[nb:nb + B * 4].view(torch.int32).tolist()
    off, base = mask_layout(Q, origs), header_bytes(B, P)
    results = []
    for b, (oh, ow) in enumerate(origs):
        res = {"boxes": boxes[b, :counts[b]]}
        if Q > 0:
            at = base + 16 * off[b]
            res["masks"] = block[at:at + Q * oh * ow].view(Q, 1, oh, ow)
        results.append(res)
    return results


def _no_targets(B, device):
    """The targets of a prediction batch as the canvas takes them: B images without boxes."""
    empty = torch.zeros((0, 4), dtype=torch.float32, device=device)
    return [{"boxes": empty} for _ in range(B)]


class _PredictStep:
    """One canvas key's capture: the StagedBatch, rt_predict_facts' table, the result block (device and pinned host) and ONE graph,
    forward -> rt_predict_canvas."""

    def __init__(self, owner, samples):
        self.owner, self.canvas, self.model, self.inner = owner, owner.canvas, owner.model, _inner(owner.model)
        img = samples["img"]
        B, dev = len(img), img.device
        self.targets = _no_targets(B, dev)
        self.staged = self.canvas.stage(samples, self.targets)          # fresh canvas-sized buffers
        self.s = self.staged.samples
        self._gen = _state(self.model).coop_generation                 # a cooperative fall-back anywhere drops this capture
        warm = []
        _warm_up(lambda: warm.append(self.model(self.s)), 1)
        P = int(warm[0]["pred_boxes"].shape[1])
        self.Q, cap = 0, 0
        if owner.segm is not None:
            pm = warm[0]["pred_masks"]
            self.Q = int(pm.shape[1])
            cap = B * 16 * -(-(self.Q * owner.max_orig[0] * owner.max_orig[1]) // 16)
        del warm
        self.B, self.P = B, P
        self.state = H.PredictState(B, P, dev, mask_capacity=cap)
        self.host = torch.empty(self.state.block.numel(), dtype=torch.uint8).pin_memory()
        self._facts(img)                                                # (the capture records the tail, it does not run it)
        self.graph = torch.cuda.CUDAGraph()
        with _capture(self.graph):
            self._tail(self.model(self.s))

    def _facts(self, img):
        origs = [(int(im.shape[0]), int(im.shape[1])) for im in img.images]
        H.predict_facts(img.out_sizes(), origs, (self.canvas.height, self.canvas.width), self.state.facts, Q=self.Q,
                        capacity=self.state.capacity)
        return origs

    def _tail(self, outputs):
        boxes = outputs["pred_boxes"]
        B, P, K, _ = boxes.shape
        pm, segm = None, self.owner.segm
        if segm is not None:
            pm = outputs["pred_masks"]
            pm = (pm.squeeze(2) if pm.dim() == 5 else pm).to(torch.float32).contiguous()
        H.predict_canvas(boxes.to(torch.float32).contiguous(), outputs["phrase_mask"].reshape(B, P, K).to(torch.uint8).contiguous(),
                         self.state, pred_masks=pm, canvas_hw=(self.canvas.height, self.canvas.width),
                         threshold=segm.threshold if segm is not None else 0.5)

    def __call__(self, samples):
        img = samples["img"]
        _before_forward_replay(self.inner)
        self.canvas.stage(samples, self.targets, out=self.staged, tokens=False)
        origs = self._facts(img)
        _copy_batch(self.s, [], {k: v for k, v in samples.items() if k != "img"}, [])
        self.graph.replay()
        used = self.state.header_bytes + 16 * mask_layout(self.Q, origs)[-1]          # known from the shapes alone
        self.host[:used].copy_(self.state.block[:used], non_blocking=True)
        torch.cuda.current_stream().synchronize()                                     # the one wait
        return decode_block(self.host, self.B, self.P, origs, self.Q)


class Predictor:
    """Applies a trained model to raw batches: `p(samples)` -> one dict per image, "boxes" fp32 [n_b, 4] (xyxy, original pixels; one
    row per valid phrase, in phrase order) and, with a 'segm' post-processor, "masks" uint8 [Q, 1, orig_h, orig_w] (0 / 1).

    `canvas`: a BatchCanvas without target masks; `max_orig_size` = (H, W): the largest original image a canvas batch may hold (it
    sizes the mask buffer: B * Q * H * W bytes on the device and in pinned memory).  A batch that fits is ONE replay of one graph per
    canvas key; the returned tensors are CPU views of the predictor's pinned result block, VALID UNTIL THE NEXT CALL (the next batch
    overwrites them: copy what must be kept), as CapturedForward's outputs are.  A batch that does not fit (`why_not`) takes the
    existing chain at its own shape and returns fresh CPU tensors of the same structure.  The model's train / eval mode is restored
    on exit.  While cooperative decoder launches are in use their failure word is read per batch; after a timed-out hand-off the
    captures are dropped and the batch runs again on the launched chain."""

    def __init__(self, model, postprocessors, canvas, max_orig_size):
        from .models.post_process import PostProcessSegm, PostProcessVGMultiPhrase
        _canvas_single_process(model)
        if torch.device(_inner(model).store.device).type != "cuda":
            raise NotImplementedError("Predictor needs the model on a GPU: there is no CPU path")
        if not (isinstance(postprocessors.get("bbox"), PostProcessVGMultiPhrase)
                and isinstance(postprocessors.get("segm", PostProcessSegm()), PostProcessSegm)):
            raise NotImplementedError("Predictor computes this package's post-processors (PostProcessVGMultiPhrase, PostProcessSegm) "
                                      "inside its graph: a foreign post-processor cannot be captured")
        if canvas.masks:
            raise ValueError("a prediction has no target masks: the canvas must be a BatchCanvas(..., masks=False)")
        self.model, self.post, self.canvas, self.segm = model, postprocessors, canvas, postprocessors.get("segm")
        self.max_orig = (int(max_orig_size[0]), int(max_orig_size[1]))
        assert self.max_orig[0] > 0 and self.max_orig[1] > 0
        self.steps = {}                          # canvas key -> _PredictStep

    def why_not(self, samples):
        """None when the batch goes through the canvas, else the reason as a short phrase: the canvas's own reasons for a raw batch
        (BatchCanvas.why_not), an original larger than max_orig_size, other token shapes than the canvas's."""
        img = samples.get("img")
        if not isinstance(img, RawImages):
            return "no RawImages"
        why = self.canvas.why_not(samples, _no_targets(len(img), "cpu"))
        if why is not None:
            return why
        for im in img.images:
            h, w = int(im.shape[0]), int(im.shape[1])
            if h > self.max_orig[0] or w > self.max_orig[1]:
                return f"original image {h} x {w} exceeds max_orig_size {self.max_orig[0]} x {self.max_orig[1]}"
        return None

    def _replay(self, key, samples):
        step = self.steps.get(key)
        if step is None:
            step = self.steps[key] = _PredictStep(self, samples)
        return step(samples)

    def _own_shape(self, samples):
        """The existing chain at the batch's own shape: resized -> the model -> the two post-processors -> the same result structure."""
        img = samples["img"]
        ns, nt = self.canvas.resized(samples, _no_targets(len(img), img.device))
        outputs = _run_again_on_chain(self.model, lambda: self.model(ns))
        orig = torch.tensor([[int(im.shape[0]), int(im.shape[1])] for im in img.images])
        scaled = self.post["bbox"](outputs, orig, scale_to_original_shape=True)
        results = [{"boxes": r["boxes"].cpu()} for r in scaled]
        if self.segm is not None:
            sizes = torch.stack([t["size"] for t in nt])
            for res, r in zip(results, self.segm([{} for _ in nt], outputs, orig, sizes)):
                res["masks"] = r["masks_origin"].cpu()
        return results

    @torch.no_grad()
    def __call__(self, samples):
        img = samples.get("img")
        if not isinstance(img, RawImages):
            raise TypeError(f"Predictor takes a raw batch: samples['img'] must be a reftr_amd.data.RawImages, not {type(img).__name__}")
        if img.gains is not None:             # (before anything is launched)
            raise ValueError("Predictor takes a raw batch without gains: the colour jitter (RawImages.gains) is a training augmentation, "
                             "and a prediction that applied it would describe another image")
        model = self.model
        was_training = model.training
        model.eval()
        try:
            if not img.is_cuda:               # a host batch: the raw bytes cross, everything else happens on the device
                samples, _ = _to_device(samples, [], _inner(model).store.device)
            if self.canvas.tokens is None:
                self.canvas.bind(samples)
            why = self.why_not(samples)
            if why is not None:
                _say_once(model, ("predict", why), f"[reftr_amd] predict: a batch does not fit {self.canvas!r} ({why}): it runs at its "
                          "own shape through the launched chain")
                return self._own_shape(samples)
            key = self.canvas.key(samples)
            if any(st._gen != _state(model).coop_generation for st in self.steps.values()):
                self.steps.clear()
            return _run_again_on_chain(model, lambda: self._replay(key, samples), drop=self.steps.clear)
        finally:
            model.train(was_training)
