"""CPU: the host side of engine_vg.evaluate_raw -- what BatchCanvas.why_not_eval_raw says, the original-frame statistics from
hand-written accumulator slots, the two rows rt_eval_raw_facts / rt_eval_orig add to the binding with every argument check that
returns before a launch, and the refusals that need no device.  Nothing here launches."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from reftr_amd import evaluate_raw, hip, metrics as M
from reftr_amd.data.canvas import BatchCanvas
from test_raw_stage_cpu import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = -1, -2


def with_ids(targets, ids, dtype=torch.int64):
    return [dict(t, image_id=torch.tensor(i, dtype=dtype)) for t, i in zip(targets, ids)]


def test_every_why_not_eval_raw_reason_fires():
    cv = BatchCanvas(144, 144, 3, masks=True)
    s, t = batch([(200, 300), (300, 200)], (1, 2))
    assert all("size" not in x and "orig_size" not in x for x in t)                   # neither is asked of a raw target
    assert cv.why_not(s, t) is None and cv.why_not_eval_raw(s, t, segm=True) is None and cv.why_not_eval_raw(s, t) is None
    assert cv.why_not_eval_raw(s, with_ids(t, (7, 9)), segm=True) is None
    assert cv.why_not_eval_raw(s, [with_ids(t, (7, 9))[0], t[1]]) == "image_id on some targets only"
    assert cv.why_not_eval_raw(s, with_ids(t, (7, 9), dtype=torch.int32)) == "an image_id that is not one int64"
    assert cv.why_not_eval_raw(s, [dict(t[0], image_id=torch.tensor([1, 2])), dict(t[1], image_id=torch.tensor([3, 4]))]) \
        == "an image_id that is not one int64"
    assert "masks=True canvas" in BatchCanvas(144, 144, 3).why_not_eval_raw(s, t, segm=True)
    assert BatchCanvas(144, 144, 3).why_not_eval_raw(s, t) is None                    # REC: the canvas needs no masks
    other = [t[0], dict(t[1], masks=torch.zeros(1, 300, 199, dtype=torch.bool))]
    assert cv.why_not_eval_raw(s, other, segm=True) == "target mask 300 x 199 on a raw image 300 x 200"
    two = [t[0], dict(t[1], masks=torch.zeros(1, 300, 200, dtype=torch.int16))]
    assert cv.why_not_eval_raw(s, two, segm=True) == "no one-byte [1, h, w] target mask"
    assert cv.why_not_eval_raw(s, two) is None                                        # without 'segm' the masks are not looked at
    flat = [t[0], dict(t[1], masks=torch.zeros(300, 200, dtype=torch.bool))]
    assert cv.why_not_eval_raw(s, flat, segm=True) == "no one-byte [1, h, w] target mask"


def test_raw_targets_restate_size_and_orig_size():
    cv = BatchCanvas(144, 144, 3, masks=True)
    s, t = batch([(200, 300), (300, 200)], (1, 2))
    full = cv.raw_targets(s, with_ids(t, (7, 9)))
    assert [x["size"].tolist() for x in full] == [[80, 120], [120, 80]] and [x["orig_size"].tolist() for x in full] == [[200, 300], [300, 200]]
    assert all(x["size"].dtype == torch.int64 and x["orig_size"].dtype == torch.int64 for x in full)
    assert [int(x["image_id"]) for x in full] == [7, 9] and full[0]["boxes"] is t[0]["boxes"] and "size" not in t[0]


def orig_slots(n=0, hit=(0,) * 5, i=0, u=0, total=0.0):
    s = [0] * hip.EVAL_ORIG_SLOTS
    s[hip.EVAL_ORIG_N], s[hip.EVAL_ORIG_I], s[hip.EVAL_ORIG_U], s[hip.EVAL_ORIG_SUM] = n, i, u, total
    s[hip.EVAL_ORIG_HIT:hip.EVAL_ORIG_HIT + 5] = hit
    return s


def test_stats_from_orig_accumulators_hand_filled():
    keys = {"seg_miou_orig", "seg_oiou_orig"} | {f"seg_prec@{t}_orig" for t in (0.5, 0.6, 0.7, 0.8, 0.9)}
    st = M.stats_from_orig_accumulators(orig_slots(n=4, hit=(4, 3, 2, 1, 0), i=300, u=1200, total=2.5))
    assert set(st) == keys
    assert st["seg_miou_orig"] == 2.5 / 4 and st["seg_oiou_orig"] == 300 / 1200
    assert [st[f"seg_prec@{t}_orig"] for t in (0.5, 0.6, 0.7, 0.8, 0.9)] == [1.0, 0.75, 0.5, 0.25, 0.0]
    # a sample whose masks were both empty: its IoU is NaN, the sum is NaN, it is a miss at every threshold
    st = M.stats_from_orig_accumulators(orig_slots(n=2, hit=(1, 1, 0, 0, 0), i=10, u=20, total=float("nan")))
    assert math.isnan(st["seg_miou_orig"]) and st["seg_oiou_orig"] == 0.5 and st["seg_prec@0.5_orig"] == 0.5
    # zero union over the whole evaluation: oIoU is NaN; zero samples: the count is clamped to 1
    st = M.stats_from_orig_accumulators(orig_slots(n=1, total=float("nan")))
    assert math.isnan(st["seg_oiou_orig"]) and math.isnan(st["seg_miou_orig"]) and st["seg_prec@0.9_orig"] == 0.0
    st = M.stats_from_orig_accumulators(orig_slots())
    assert set(st) == keys and st["seg_miou_orig"] == 0.0 and math.isnan(st["seg_oiou_orig"]) and st["seg_prec@0.5_orig"] == 0.0


def test_meter_carries_the_orig_slots_beside_acc():
    m = M.EvalMeter("cpu", seg=True)
    assert m.acc.numel() == hip.EVAL_SLOTS and m.acc_orig.numel() == hip.EVAL_ORIG_SLOTS
    assert m.acc_orig.data_ptr() == m.acc.data_ptr() + 8 * hip.EVAL_SLOTS             # one block: one zeroing, one copy
    m.acc_orig[hip.EVAL_ORIG_N], m.acc_orig[hip.EVAL_ORIG_I], m.acc_orig[hip.EVAL_ORIG_U] = 2, 3, 4
    m.acc_orig[hip.EVAL_ORIG_SUM:].view(torch.float64)[0] = 1.5
    assert not any(k.endswith("_orig") for k in m.compute())                          # nobody booked the original-frame totals
    m.book_orig()
    st = m.compute()
    assert st["seg_miou_orig"] == 0.75 and st["seg_oiou_orig"] == 0.75 and "seg_miou" in st
    m.reset()
    assert not bool(m.acc_orig.any()) and not any(k.endswith("_orig") for k in m.compute())


def test_abi_rows_and_argument_blocks():
    header = open(os.path.join(ROOT, "include", "reftr_hip.h")).read()
    assert hip.ABI_VERSION == 39                                                      # purely additive
    assert re.search(r"\bint rt_eval_raw_facts\(const rt_eval_raw_facts_args\* a, rt_stream_t stream\);", header)
    assert re.search(r"\bint rt_eval_orig\(const rt_eval_orig_args\* a, rt_stream_t stream\);", header)
    for name, value in (("N", 0), ("HIT", 1), ("I", 6), ("U", 7), ("SUM", 8), ("SLOTS", 9)):
        assert re.search(r"#define RT_EVAL_ORIG_%s %d\b" % (name, value), header) and getattr(hip, "EVAL_ORIG_" + name) == value
    for name, cls in (("rt_eval_raw_facts", hip.EvalRawFactsArgs), ("rt_eval_orig", hip.EvalOrigArgs)):
        res, args = hip._SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.POINTER(cls), ctypes.c_void_p]
        assert hip.STRUCTS[name + "_args"] is cls
    # everything rides by value: the struct is the kernel's only argument and stays under the launch's 4 KB
    n = hip.BATCH_STAGE_MAX_B
    assert ctypes.sizeof(hip.EvalRawFactsArgs) == 48 + (4 * 4 + 8 + 8) * n <= 4096
    assert all(getattr(hip.EvalRawFactsArgs, f).size == n * (8 if f in ("image_id", "tm_ptr") else 4)
               for f in ("img_h", "img_w", "orig_h", "orig_w", "image_id", "tm_ptr"))
    assert ctypes.sizeof(hip.EvalOrigArgs) + 1 * 4 <= 4096
    a = hip._desc(hip.EvalRawFactsArgs, B=2, max_pixels=1 << 33, img_h=[5, 7], image_id=[1 << 40], tm_ptr=[None, None])
    assert list(a.img_h)[:3] == [5, 7, 0] and a.image_id[0] == 1 << 40 and a.max_pixels == 1 << 33 and a.mask_table is None
    assert hip.eval_orig_chunks(16 * 640 * 640) == 400 and hip.eval_orig_chunks(16385) == 2 and hip.eval_orig_chunks(1) == 1


def test_argument_checks_return_before_any_launch():
    """Every RT_ERR_BADARG / RT_ERR_UNSUPPORTED case of the two entry points: decided on the host from the argument block alone (the
    pointers are never followed), so no device is needed."""
    L, n = hip.lib(), hip.BATCH_STAGE_MAX_B
    arr = lambda v: (ctypes.c_int32 * n)(*v)
    FAKE = 0x1000                                                                     # non-NULL, never dereferenced

    def facts(**kw):
        f = dict(facts=FAKE, image_ids=FAKE, mask_table=FAKE, max_pixels=16 * 96 * 128, B=2, Hc=96, Wc=128, has_ids=1,
                 img_h=arr([75, 96]), img_w=arr([100, 128]), orig_h=arr([75, 37]), orig_w=arr([100, 51]),
                 image_id=(ctypes.c_int64 * n)(5, 6), tm_ptr=(ctypes.c_void_p * n)(FAKE, FAKE))
        f.update(kw)
        return L.rt_eval_raw_facts(ctypes.byref(hip.EvalRawFactsArgs(**f)), None)
    assert L.rt_eval_raw_facts(None, None) == BAD
    for kw in (dict(facts=None), dict(image_ids=None), dict(B=0), dict(B=-1), dict(Hc=0), dict(Wc=-2),
               dict(img_h=arr([0, 96])), dict(img_w=arr([100, -3])), dict(orig_h=arr([75, 0])), dict(orig_w=arr([0, 51])),
               dict(img_h=arr([97, 96])), dict(img_w=arr([100, 129])),                 # larger than the canvas
               dict(max_pixels=7499), dict(max_pixels=0), dict(orig_h=arr([75, 4000]), orig_w=arr([100, 4000])),   # more than max_pixels
               dict(tm_ptr=(ctypes.c_void_p * n)(FAKE, None))):                        # a table, and a mask pointer missing
        assert facts(**kw) == BAD, kw
    assert facts(B=n + 1) == UNSUPPORTED and facts(max_pixels=1 << 31) == UNSUPPORTED and facts(max_pixels=1 << 40) == UNSUPPORTED

    def orig(**kw):
        f = dict(pred_masks=FAKE, facts=FAKE, mask_table=FAKE, partials=FAKE, iou_seg=FAKE, iu=FAKE, acc=FAKE, veto=None,
                 max_pixels=16 * 96 * 128, B=2, Q=2, h=24, w=32, Hc=96, Wc=128, threshold=0.5)
        f.update(kw)
        return L.rt_eval_orig(ctypes.byref(hip.EvalOrigArgs(**f)), None)
    assert L.rt_eval_orig(None, None) == BAD
    for name in ("pred_masks", "facts", "mask_table", "partials", "iou_seg", "iu", "acc"):
        assert orig(**{name: None}) == BAD, name
    for name in ("B", "Q", "h", "w", "Hc", "Wc", "max_pixels"):
        assert orig(**{name: 0}) == BAD and orig(**{name: -1}) == BAD, name
    assert orig(B=n + 1) == UNSUPPORTED and orig(max_pixels=1 << 31) == UNSUPPORTED
    assert orig(h=1 << 16, w=1 << 15) == UNSUPPORTED and orig(Hc=1 << 16, Wc=1 << 15) == UNSUPPORTED


class _Model(torch.nn.Module):
    def __init__(self, device="cuda"):
        super().__init__()
        self.store = SimpleNamespace(device=torch.device(device))


class _Criterion(torch.nn.Module):
    targets_static = target_masks_static = None
    weight_dict = {}


def _post():
    from reftr_amd.models.post_process import PostProcessVGMultiPhrase
    return {"bbox": PostProcessVGMultiPhrase()}


def test_refusals_that_need_no_device(monkeypatch):
    from reftr_amd.util.misc import NestedTensor
    cv = BatchCanvas(144, 144, 3)
    loader = [batch([(200, 300), (300, 200)], (1, 2))]
    model, crit = _Model(), _Criterion()
    model.train(); crit.train()
    with pytest.raises(NotImplementedError, match="a CPU device"):
        evaluate_raw(model, crit, _post(), loader, torch.device("cpu"), cv)
    with pytest.raises(NotImplementedError, match="post-processor"):
        evaluate_raw(model, crit, {"bbox": torch.nn.Identity()}, loader, torch.device("cuda"), cv)
    with pytest.raises(NotImplementedError, match="post-processor"):
        evaluate_raw(model, crit, dict(_post(), segm=torch.nn.Identity()), loader, torch.device("cuda"), cv)
    with pytest.raises(NotImplementedError, match="targets_static"):
        evaluate_raw(model, torch.nn.Identity(), _post(), loader, torch.device("cuda"), cv)
    wrapped = torch.nn.Module()
    wrapped.module = model
    with pytest.raises(NotImplementedError, match="data-parallel"):
        evaluate_raw(wrapped, crit, _post(), loader, torch.device("cuda"), cv)
    with pytest.raises(NotImplementedError, match="needs a canvas"):
        evaluate_raw(model, crit, _post(), loader, torch.device("cuda"), None)
    for switch in ("REFTR_EVAL_GRAPH", "REFTR_EVAL_METRICS"):
        monkeypatch.setenv(switch, "0")
        with pytest.raises(NotImplementedError, match=switch + "=0"):
            evaluate_raw(model, crit, _post(), loader, torch.device("cuda"), cv)
        monkeypatch.delenv(switch)
    s, t = loader[0]
    nested = dict(s, img=NestedTensor(torch.zeros(2, 3, 96, 128), torch.zeros(2, 96, 128, dtype=torch.bool)))
    with pytest.raises(TypeError, match="RawImages"):
        evaluate_raw(model, crit, _post(), [(nested, t)], torch.device("cuda"), cv)
    assert model.training and crit.training                                            # nothing was touched
