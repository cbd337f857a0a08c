"""CPU: the host side of a canvas evaluation -- metrics.decode_ring on numpy arrays and BatchCanvas.why_not_eval on CPU tensors."""
import numpy as np
import pytest
import torch

from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.metrics import decode_ring
from reftr_amd.util.misc import NestedTensor


def _ring(slots=3, B=2, P=4, seed=0):
    rng = np.random.default_rng(seed)
    boxes = rng.uniform(0, 700, size=(slots, B, P, 4)).astype(np.float32)
    counts = np.array([[2, 0], [4, 1], [3, 3]], dtype=np.int32)[:slots]
    ids = np.array([[7, 8], [2 ** 53 - 1, 11], [12, 13]], dtype=np.int64)[:slots]
    return boxes, counts, ids


def test_decode_keys_nesting_and_exact_values():
    boxes, counts, ids = _ring()
    batches = [(0, True, [2, 0]), (2, True, [4, 1]), (5, True, [3, 3])]
    frags = decode_ring(boxes, counts, ids, 3, 0, batches)
    assert [sorted(f) for f in frags] == [[7, 8], [11, 2 ** 53 - 1], [12, 13]]             # one dict per slot, int keys
    assert all(type(k) is int for f in frags for k in f)
    assert frags[0][8] == [] and len(frags[1][2 ** 53 - 1]) == 4 and len(frags[1][2 ** 53 - 1][0]) == 4
    for slot, f in enumerate(frags):
        for b in range(2):
            rows = f[int(ids[slot, b])]
            assert all(type(v) is float for r in rows for v in r)
            # float64 holds every fp32 coordinate exactly: what .cpu().numpy().tolist() of the fp32 boxes gives
            assert rows == boxes[slot, b, :counts[slot, b]].tolist()
            assert np.array_equal(np.asarray(rows, dtype=np.float32).reshape(-1, 4), boxes[slot, b, :counts[slot, b]])


def test_decode_skips_images_without_image_id():
    boxes, counts, ids = _ring()
    frags = decode_ring(boxes, counts, ids, 3, 0, [(0, True, [2, 0]), (1, False, [4, 1]), (2, True, [3, 3])])
    assert frags[1] == {} and sorted(frags[0]) == [7, 8] and sorted(frags[2]) == [12, 13]


def test_decode_count_mismatch_names_batch_and_image():
    boxes, counts, ids = _ring()
    with pytest.raises(AssertionError, match=r"batch 5, image 1: 3 result boxes for 2 target boxes"):
        decode_ring(boxes, counts, ids, 3, 0, [(0, True, [2, 0]), (2, True, [4, 1]), (5, True, [3, 2])])
    with pytest.raises(AssertionError, match=r"batch 1, image 0"):                         # also for a batch without ids
        decode_ring(boxes, counts, ids, 3, 0, [(0, True, [2, 0]), (1, False, [1, 1]), (2, True, [3, 3])])


def test_decode_overflow_and_short_cursor_raise():
    boxes, counts, ids = _ring()
    batches = [(0, True, [2, 0]), (1, True, [4, 1]), (2, True, [3, 3])]
    with pytest.raises(RuntimeError, match="overflowed"):
        decode_ring(boxes, counts, ids, 3, 1, batches)
    with pytest.raises(RuntimeError, match="holds 2 batches, 3 were replayed"):
        decode_ring(boxes, counts, ids, 2, 0, batches)


def _batch(B=2, h=64, w=96, masks=True):
    samples = {"img": NestedTensor(torch.zeros(B, 3, h, w), torch.zeros(B, h, w, dtype=torch.bool)),
               "sentence": torch.zeros(B, 12, dtype=torch.long)}
    targets = [{"boxes": torch.rand(1, 4), "labels": torch.zeros(1, dtype=torch.long), "size": torch.tensor([h, w]),
                "orig_size": torch.tensor([2 * h, 2 * w]), "image_id": torch.tensor(b)} for b in range(B)]
    if masks:
        for t in targets:
            t["masks"] = torch.zeros(1, h, w, dtype=torch.bool)
    return samples, targets


def test_eval_fit_reasons_one_by_one():
    cv = BatchCanvas(128, 128, 2, masks=True)
    s, t = _batch()
    assert cv.why_not(s, t) is None and cv.why_not_eval(s, t, segm=True) is None and cv.why_not_eval(s, t) is None
    assert BatchCanvas(128, 128, 2).why_not_eval(s, t, segm=True) == "a 'segm' post-processor needs a masks=True canvas"

    def reason(change, segm=True):
        s, t = _batch()
        change(t)
        return cv.why_not_eval(s, t, segm=segm)
    assert reason(lambda t: t[1].pop("size")) == "no int64 [2] size on a target"
    assert reason(lambda t: t[0].update(size=torch.tensor([64.0, 96.0]))) == "no int64 [2] size on a target"
    assert reason(lambda t: t[0].update(size=torch.tensor([64, 96, 3]))) == "no int64 [2] size on a target"
    assert reason(lambda t: t[1].pop("orig_size")) == "no int64 [2] orig_size on a target while another has one"
    assert reason(lambda t: [x.pop("orig_size") for x in t]) is None                          # none has it: the size is used
    assert reason(lambda t: t[0].pop("image_id")) == "image_id on some targets only"
    assert reason(lambda t: [x.pop("image_id") for x in t]) is None                           # all or none
    assert reason(lambda t: t[1].update(image_id=torch.tensor([1, 2]))) == "an image_id that is not one int64"
    assert reason(lambda t: t[1].pop("masks")) == "no one-byte [1, h, w] target mask"
    assert reason(lambda t: t[1].update(masks=torch.zeros(1, 64, 96))) == "no one-byte [1, h, w] target mask"
    assert reason(lambda t: t[1].update(masks=torch.zeros(64, 96, dtype=torch.uint8))) == "no one-byte [1, h, w] target mask"
    assert reason(lambda t: t[1].pop("masks"), segm=False) is None                            # REC: no mask is asked for
    # training's conditions are separate and unchanged: a target without `size` still fits a training step
    s, t = _batch()
    t[0].pop("size")
    assert cv.why_not(s, t) is None
