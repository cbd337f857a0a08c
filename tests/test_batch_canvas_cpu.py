"""CPU: the batch canvas's host side -- pad_on_host against the reference-style collate, fits(), the capture key."""
import types

import torch

from oracle.synth import make_inputs
from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.util.misc import NestedTensor, nested_tensor_from_tensor_list


def batch(H, W, L=12, n_phrase=3, counts=(3, 2), mask_hw=None, name="canvas_cpu"):
    """A make_inputs batch as the engine sees it; image b keeps `counts[b]` boxes and, with mask_hw, gets a [1, h, w] target mask."""
    samples, targets = make_inputs(name, B=len(counts), H=H, W=W, L=L, n_phrase=n_phrase)
    s = {k: v for k, v in samples.items() if k not in ("img", "img_mask")}
    s["img"] = NestedTensor(samples["img"], samples["img_mask"])
    gen = torch.Generator().manual_seed(H * 1000 + W)
    out = []
    for b, n in enumerate(counts):
        bx = torch.rand(n, 4, generator=gen) * 0.4 + 0.3
        t = {"boxes": bx, "labels": torch.zeros(n, dtype=torch.long)}
        if mask_hw is not None:
            h, w = mask_hw[b]
            t["masks"] = torch.rand(1, h, w, generator=gen) < 0.5
        out.append(t)
    return s, out


def test_pad_on_host_is_the_collate_with_one_canvas_sized_image():
    cv = BatchCanvas(16, 20, 3, masks=True)
    s, t = batch(11, 14, mask_hw=[(11, 14), (5, 9)])
    ps, pt = cv.pad_on_host(s, t)
    # util/collate_fn.py:24-41 pads to the largest image of the batch: append one zero image of canvas size, collate, drop it
    imgs = [im for im in s["img"].tensors] + [torch.zeros(3, 16, 20)]
    ref = nested_tensor_from_tensor_list(imgs)
    assert torch.equal(ps["img"].tensors, ref.tensors[:2])
    # the collate marks what it padded; what the batch's own mask already marked stays marked
    want = ref.mask[:2].clone()
    want[:, :11, :14] |= s["img"].mask
    assert ps["img"].mask.dtype == torch.bool and torch.equal(ps["img"].mask, want)
    assert ps["img"].mask[:, 11:, :].all() and ps["img"].mask[:, :, 14:].all()
    # target masks: the zero-padded batch of nested_tensor_from_tensor_list (util/misc.py:288-305) with a canvas-sized entry
    for b, (h, w) in enumerate([(11, 14), (5, 9)]):
        m = pt[b]["masks"]
        assert tuple(m.shape) == (1, 16, 20) and m.dtype == t[b]["masks"].dtype
        assert torch.equal(m[:, :h, :w], t[b]["masks"]) and not m[:, h:, :].any() and not m[:, :, w:].any()
        assert torch.equal(pt[b]["boxes"], t[b]["boxes"]) and torch.equal(pt[b]["labels"], t[b]["labels"])
    for k in ("sentence", "sentence_mask", "phrase", "phrase_mask"):
        assert torch.equal(ps[k], s[k])
    # a batch of canvas size comes back unchanged
    s2, t2 = batch(16, 20, mask_hw=[(16, 20), (16, 20)])
    p2, q2 = cv.pad_on_host(s2, t2)
    assert torch.equal(p2["img"].tensors, s2["img"].tensors) and torch.equal(p2["img"].mask, s2["img"].mask)
    assert all(torch.equal(a["masks"], b["masks"]) for a, b in zip(q2, t2))


def test_fits_accepts_and_refuses():
    s, t = batch(16, 20)
    cv = BatchCanvas(16, 20, 3).bind(s)
    assert cv.fits(s, t)
    assert cv.fits(*batch(1, 1, counts=(0, 0)))
    assert cv.fits(*batch(16, 3, counts=(3, 3)))
    assert not cv.fits(*batch(17, 20)) and "exceeds" in cv.why_not(*batch(17, 20))          # one pixel too tall
    assert not cv.fits(*batch(16, 21))
    assert not cv.fits(*batch(16, 20, counts=(3, 4))) and "boxes" in cv.why_not(*batch(16, 20, counts=(3, 4)))      # one box too many
    assert not cv.fits(*batch(16, 20, L=10)) and "token" in cv.why_not(*batch(16, 20, L=10))                         # another sentence length
    assert not cv.fits(*batch(16, 20, n_phrase=2, counts=(2, 2)))
    cm = BatchCanvas(16, 20, 3, masks=True).bind(s)
    assert cm.fits(*batch(8, 8, mask_hw=[(16, 20), (1, 1)]))
    assert not cm.fits(*batch(8, 8, mask_hw=[(17, 20), (1, 1)]))
    assert not cm.fits(*batch(8, 8))                                                          # no masks at all


def test_from_args():
    s, _ = batch(16, 20)
    cv = BatchCanvas.from_args(types.SimpleNamespace(max_img_size=640, masks=False), s)
    assert (cv.height, cv.width, cv.boxes_per_image, cv.masks) == (640, 640, 3, False) and cv.tokens is not None
    one = {k: v for k, v in s.items() if not k.startswith("phrase")}
    assert BatchCanvas.from_args(types.SimpleNamespace(max_img_size=512, masks=True), one).boxes_per_image == 1


def test_capture_key():
    cv = BatchCanvas(16, 20, 3, masks=True)
    a = batch(16, 20, counts=(3, 2), mask_hw=[(16, 20), (16, 20)])
    b = batch(9, 20, counts=(0, 3), mask_hw=[(3, 4), (9, 20)])
    assert cv.key(a[0]) == cv.key(b[0])                                   # image size, box counts, mask sizes: not in the key
    from reftr_amd.engine_vg import CapturedTrainStep
    assert CapturedTrainStep.shape_key(*a) != CapturedTrainStep.shape_key(*b)       # ... while the shape key has them all
    assert cv.key(batch(16, 20, counts=(3, 2, 1))[0]) != cv.key(a[0])                # B
    assert cv.key(batch(16, 20, L=10)[0]) != cv.key(a[0])                            # token lengths
    assert cv.key(batch(16, 20, n_phrase=4, counts=(3, 2))[0]) != cv.key(a[0])
    for other in (BatchCanvas(16, 24, 3, masks=True), BatchCanvas(20, 20, 3, masks=True), BatchCanvas(16, 20, 4, masks=True),
                  BatchCanvas(16, 20, 3)):
        assert other.key(a[0]) != cv.key(a[0])                                       # the canvas
    hash(cv.key(a[0]))
