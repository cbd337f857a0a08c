"""CPU: the host side of raw batches -- RawImages / raw_collate, what BatchCanvas says about them (key, why_not) and rt_raw_stage's row
of the binding.  Nothing here launches: shapes, dtypes and host integers only."""
import ctypes
import os
import re

import torch

from reftr_amd import hip
from reftr_amd.data import RawImages, raw_collate, resample
from reftr_amd.data.canvas import BatchCanvas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def item(h, w, n_boxes, L=5, mask=True):
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8)
    fields = {"sentence": torch.arange(L), "sentence_mask": torch.ones(L, dtype=torch.bool)}
    target = {"boxes": torch.rand(n_boxes, 4) * torch.tensor([w, h, w, h]), "labels": torch.zeros(n_boxes, dtype=torch.long)}
    if mask:
        target["masks"] = torch.zeros(1, h, w, dtype=torch.bool)
    return img, fields, target


def batch(sizes, counts, size=80, max_size=144, **kw):
    return raw_collate(size, max_size)([item(h, w, n, **kw) for (h, w), n in zip(sizes, counts)])


def test_raw_collate_shapes_and_to():
    s, t = batch([(200, 300), (300, 200), (31, 47)], (0, 1, 3))
    img = s["img"]
    assert isinstance(img, RawImages) and len(img) == 3 and (img.size, img.max_size) == (80, 144)
    assert [tuple(im.shape) for im in img.images] == [(200, 300, 3), (300, 200, 3), (31, 47, 3)]
    assert all(im.dtype == torch.uint8 for im in img.images) and img.well_formed() and not img.is_cuda
    assert tuple(s["sentence"].shape) == (3, 5) and tuple(s["sentence_mask"].shape) == (3, 5)
    assert [tuple(x["boxes"].shape) for x in t] == [(0, 4), (1, 4), (3, 4)] and tuple(t[0]["masks"].shape) == (1, 200, 300)
    # the resized sizes are resample.size_with_aspect_ratio's, the single definition
    assert img.out_sizes() == [(80, 120), (120, 80), (80, 121)]
    assert img.out_sizes() == [resample.size_with_aspect_ratio(im.shape[1], im.shape[0], 80, 144) for im in img.images]
    moved = img.to("cpu", non_blocking=True)
    assert isinstance(moved, RawImages) and (moved.size, moved.max_size) == (80, 144) and moved.out_sizes() == img.out_sizes()
    assert all(torch.equal(a, b) for a, b in zip(moved.images, img.images)) and moved.device.type == "cpu"
    moved.record_stream(None)                                # host tensors: nothing to record
    # what the engine's prefetcher does to a batch moves a RawImages like any other field
    from reftr_amd.engine_vg import _to_device
    s2, t2 = _to_device(s, t, torch.device("cpu"))
    assert isinstance(s2["img"], RawImages) and torch.equal(s2["sentence"], s["sentence"]) and torch.equal(t2[2]["boxes"], t[2]["boxes"])


def test_canvas_key_does_not_depend_on_image_sizes():
    cv = BatchCanvas(144, 144, 3, masks=True)
    a, _ = batch([(200, 300), (300, 200)], (1, 1))
    b, _ = batch([(31, 47), (80, 120)], (3, 0))
    c, _ = batch([(31, 47), (80, 120), (80, 120)], (3, 0, 0))
    d, _ = batch([(31, 47), (80, 120)], (3, 0), L=7)
    assert cv.key(a) == cv.key(b) and cv.key(a)[0] == "canvas"
    assert cv.key(c) != cv.key(a) and cv.key(d) != cv.key(a)           # the batch size and the token shapes do count


def test_raw_batches_that_fit():
    cv = BatchCanvas(144, 144, 3, masks=True)
    s, t = batch([(200, 300), (300, 200), (256, 400), (31, 47), (80, 120)], (0, 1, 3, 2, 1))
    assert cv.why_not(s, t) is None and cv.fits(s, t)
    s, t = batch([(320, 480)], (1,))                         # exactly the limit: 320 / 80 = 480 / 120 = 4
    assert s["img"].out_sizes() == [(80, 120)] and cv.why_not(s, t) is None


def test_every_new_reason_fires():
    cv = BatchCanvas(144, 144, 3, masks=True)
    s, t = batch([(200, 300), (300, 200)], (1, 1))
    bad = dict(s, img=RawImages([s["img"].images[0], s["img"].images[1].float()], 80, 144))
    assert "not uint8 [h, w, 3]" in cv.why_not(bad, t)
    bad = dict(s, img=RawImages([s["img"].images[0], s["img"].images[1][:, :, :2]], 80, 144))
    assert "not uint8 [h, w, 3]" in cv.why_not(bad, t)
    bad = dict(s, img=RawImages([s["img"].images[0], s["img"].images[1].permute(2, 0, 1)], 80, 144))
    assert "not uint8 [h, w, 3]" in cv.why_not(bad, t)
    # 200 x 300 at size 120 / max_size 180 -> 120 x 180: wider than the canvas
    bad = dict(s, img=RawImages(s["img"].images, 120, 180))
    assert bad["img"].out_sizes()[0] == (120, 180) and "exceeds the canvas" in cv.why_not(bad, t)
    # 400 x 600 -> 80 x 120: a down-scale by 5, the kernel's limit is RT_RAW_STAGE_MAX_SCALE = 4
    s5, t5 = batch([(200, 300), (400, 600)], (1, 1))
    assert hip.RAW_STAGE_MAX_SCALE == 4 and s5["img"].out_sizes()[1] == (80, 120)
    assert "scaled down by more than 4" in cv.why_not(s5, t5) and not cv.fits(s5, t5)
    tm = [dict(t[0]), dict(t[1], masks=torch.zeros(1, 300, 199, dtype=torch.bool))]
    assert "target mask 300 x 199 on a raw image 300 x 200" in cv.why_not(s, tm)
    assert BatchCanvas(144, 144, 3).why_not(s, tm) is None                    # a canvas without masks does not look at them
    # ... and the reasons the two forms of a batch share
    assert "capacity 3" in cv.why_not(*batch([(200, 300)], (4,)))
    assert "no [1, h, w] target mask" in cv.why_not(*batch([(200, 300)], (1,), mask=False))
    assert "targets do not match" in cv.why_not(s, t[:1])
    bound = BatchCanvas(144, 144, 3, masks=True).bind(s)
    assert bound.why_not(s, t) is None and "token field shapes" in bound.why_not(*batch([(200, 300), (300, 200)], (1, 1), L=7))


def test_nested_batches_are_judged_as_before():
    from reftr_amd.util.misc import NestedTensor
    cv = BatchCanvas(144, 144, 3)
    s = {"img": NestedTensor(torch.zeros(2, 3, 96, 128), torch.zeros(2, 96, 128, dtype=torch.bool)), "sentence": torch.zeros(2, 5)}
    t = [{"boxes": torch.rand(1, 4)}, {"boxes": torch.rand(2, 4)}]
    assert cv.why_not(s, t) is None and cv.key(s) == ("canvas", 144, 144, 3, False, 2, (("sentence", (5,)),))
    s["img"] = NestedTensor(torch.zeros(2, 3, 96, 160), torch.zeros(2, 96, 160, dtype=torch.bool))
    assert cv.why_not(s, t) == "image 96 x 160 exceeds the canvas"


def test_abi_row_and_argument_block():
    header = open(os.path.join(ROOT, "include", "reftr_hip.h")).read()
    assert hip.ABI_VERSION == 39
    assert re.search(r"\bint rt_raw_stage\(const rt_raw_stage_args\* a, rt_stream_t stream\);", header)
    assert re.search(r"\bint rt_resample_taps\(", header) and "#define RT_RAW_STAGE_MAX_SCALE 4" in header
    res, args = hip._SIGNATURES["rt_raw_stage"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(hip.RawStageArgs), ctypes.c_void_p]
    assert len(hip._SIGNATURES["rt_resample_taps"][1]) == 6
    assert hip.STRUCTS["rt_raw_stage_args"] is hip.RawStageArgs
    # everything rides by value in the launch's argument block: the struct plus the kernel's five words stay under its 4 KB
    n = hip.BATCH_STAGE_MAX_B
    assert ctypes.sizeof(hip.RawStageArgs) + 5 * 4 <= 4096
    assert all(getattr(hip.RawStageArgs, f).size == n * (8 if f in ("src", "box_ptr", "tm_ptr") else 4)
               for f in ("src", "box_ptr", "tm_ptr", "h", "w", "oh", "ow", "box_n", "rw", "rh"))
    a = hip._desc(hip.RawStageArgs, B=2, h=[5, 7], rw=[0.5], src=[None, None], mean=(1.0, 2.0, 3.0))
    assert list(a.h)[:3] == [5, 7, 0] and a.rw[0] == 0.5 and list(a.mean) == [1.0, 2.0, 3.0] and a.tm_ptr[0] is None


def test_a_raw_batch_needs_a_canvas():
    import pytest
    from reftr_amd.engine_vg import begin_train_step, train_step
    s, t = batch([(200, 300)], (1,))
    for fn in (train_step, begin_train_step):
        with pytest.raises(NotImplementedError, match="needs canvas="):
            fn(torch.nn.Identity(), None, s, t, None)
