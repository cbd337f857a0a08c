"""CPU: the host side of prediction (reftr_amd/predict.py) -- the packed mask layout, the decode of a result block, what
Predictor.why_not says, the refusals that need no device, and the two rows rt_predict_facts / rt_predict_canvas add to the binding.
Nothing here launches."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from reftr_amd import Predictor, hip
from reftr_amd.data import RawImages
from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.predict import decode_block, header_bytes, mask_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_layout_by_hand():
    """Q = 2: 2 * 37 * 51 = 3774 bytes -> 236 units (3776 bytes: a tail of 2); 2 * 1 * 17 = 34 -> 3 units; 2 * 4 * 8 = 64 -> exactly 4."""
    assert mask_layout(2, [(37, 51), (1, 17), (4, 8)]) == [0, 236, 239, 243]
    assert mask_layout(1, [(1, 1)]) == [0, 1] and mask_layout(1, [(4, 4), (4, 4)]) == [0, 1, 2]
    assert mask_layout(0, [(375, 500), (7, 9)]) == [0, 0, 0]                         # a model without masks: no bytes
    assert mask_layout(3, []) == [0]
    off = mask_layout(2, [(333, 500), (96, 128)])
    assert off == [0, 20813, 20813 + 1536] and 16 * off[1] - 2 * 333 * 500 == 8      # 333000 bytes, a tail of 8


def test_decode_of_a_packed_block():
    B, P, Q, origs = 2, 3, 2, [(2, 3), (1, 5)]
    hb = header_bytes(B, P)
    assert hb == 112 and header_bytes(1, 1) == 32 and header_bytes(4, 4) == 272        # 2 * 3 * 16 + 2 * 4 = 104 -> 112
    off = mask_layout(Q, origs)
    assert off == [0, 1, 2]
    block = torch.full((hb + 16 * off[-1],), 0xA5, dtype=torch.uint8)
    boxes = torch.arange(B * P * 4, dtype=torch.float32).view(B, P, 4) + 0.5
    block[:96] = boxes.view(-1).view(torch.uint8)
    block[96:104] = torch.tensor([2, 0], dtype=torch.int32).view(torch.uint8)
    m0 = torch.tensor([1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1], dtype=torch.uint8)
    m1 = torch.tensor([0, 1, 0, 1, 0, 1, 1, 1, 1, 0], dtype=torch.uint8)
    block[hb:hb + 12], block[hb + 16:hb + 26] = m0, m1
    res = decode_block(block, B, P, origs, Q)
    assert len(res) == 2 and torch.equal(res[0]["boxes"], boxes[0, :2]) and tuple(res[1]["boxes"].shape) == (0, 4)
    assert tuple(res[0]["masks"].shape) == (2, 1, 2, 3) and torch.equal(res[0]["masks"].reshape(-1), m0)
    assert tuple(res[1]["masks"].shape) == (2, 1, 1, 5) and torch.equal(res[1]["masks"].reshape(-1), m1)
    assert res[0]["masks"][1, 0].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert res[0]["masks"].data_ptr() == block.data_ptr() + hb                       # views of the block, no copies
    assert res[1]["masks"].data_ptr() == block.data_ptr() + hb + 16
    assert "masks" not in decode_block(block, B, P, origs)[0]                         # Q = 0: REC


def test_abi_rows_and_argument_block():
    header = open(os.path.join(ROOT, "include", "reftr_hip.h")).read()
    assert hip.ABI_VERSION == 39                                                      # purely additive
    assert re.search(r"\bint rt_predict_facts\(const rt_predict_facts_args\* a, rt_stream_t stream\);", header)
    assert re.search(r"\bint rt_predict_canvas\(const rt_predict_canvas_args\* a, rt_stream_t stream\);", header)
    assert "#define RT_PREDICT_FACTS_WORDS 8" in header and hip.PREDICT_FACTS_WORDS == 8
    for name, cls in (("rt_predict_facts", hip.PredictFactsArgs), ("rt_predict_canvas", hip.PredictCanvasArgs)):
        res, args = hip._SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.POINTER(cls), ctypes.c_void_p]
        assert hip.STRUCTS[name + "_args"] is cls
    # rt_predict_facts' sizes ride by value: the struct is the kernel's only argument and stays under the launch's 4 KB
    n = hip.BATCH_STAGE_MAX_B
    assert ctypes.sizeof(hip.PredictFactsArgs) + 0 * 4 <= 4096 and ctypes.sizeof(hip.PredictFactsArgs) == 32 + 4 * 4 * n
    assert all(getattr(hip.PredictFactsArgs, f).size == 4 * n for f in ("img_h", "img_w", "orig_h", "orig_w"))
    assert ctypes.sizeof(hip.PredictCanvasArgs) + 1 * 4 <= 4096
    a = hip._desc(hip.PredictFactsArgs, B=2, Q=1, capacity=1 << 33, img_h=[5, 7], orig_w=[9])
    assert list(a.img_h)[:3] == [5, 7, 0] and a.orig_w[0] == 9 and a.capacity == 1 << 33 and a.facts is None


class _Model(torch.nn.Module):
    """What Predictor looks at before anything is launched: the parameter store's device, and the train / eval mode."""

    def __init__(self, device="cuda"):
        super().__init__()
        self.store = SimpleNamespace(device=torch.device(device))


def _post(segm=False):
    from reftr_amd.models.post_process import PostProcessSegm, PostProcessVGMultiPhrase
    return {"bbox": PostProcessVGMultiPhrase(), "segm": PostProcessSegm()} if segm else {"bbox": PostProcessVGMultiPhrase()}


def _samples(sizes, size=80, max_size=144, L=5):
    B = len(sizes)
    return {"img": RawImages([torch.zeros((h, w, 3), dtype=torch.uint8) for h, w in sizes], size, max_size),
            "sentence": torch.zeros(B, L, dtype=torch.long), "sentence_mask": torch.ones(B, L, dtype=torch.bool)}


def test_every_why_not_reason_fires():
    good = _samples([(200, 300), (300, 200)])
    p = Predictor(_Model(), _post(True), BatchCanvas(144, 144, 1).bind(good), max_orig_size=(300, 300))
    assert p.why_not(good) is None
    assert p.why_not(_samples([(31, 47), (80, 120)])) is None                         # other image sizes: the same canvas
    # the canvas's raw reasons
    bad = dict(good, img=RawImages([good["img"].images[0], good["img"].images[1].float()], 80, 144))
    assert "not uint8 [h, w, 3]" in p.why_not(bad)
    bad = dict(good, img=RawImages(good["img"].images, 120, 180))                     # 200 x 300 -> 120 x 180
    assert "exceeds the canvas" in p.why_not(bad)
    wide = Predictor(_Model(), _post(True), BatchCanvas(144, 144, 1), max_orig_size=(600, 600))
    assert "scaled down by more than 4" in wide.why_not(_samples([(200, 300), (400, 600)]))
    assert "more than 64 images" in wide.why_not(_samples([(20, 30)] * 65))
    # an original larger than max_orig_size (either axis)
    assert p.why_not(_samples([(200, 300), (301, 200)])) == "original image 301 x 200 exceeds max_orig_size 300 x 300"
    assert "original image 200 x 301" in p.why_not(_samples([(200, 301), (100, 100)]))
    # other token shapes than the canvas's
    assert "token field shapes" in p.why_not(_samples([(200, 300), (300, 200)], L=7))
    # not a raw batch at all
    from reftr_amd.util.misc import NestedTensor
    nested = dict(good, img=NestedTensor(torch.zeros(2, 3, 96, 128), torch.zeros(2, 96, 128, dtype=torch.bool)))
    assert p.why_not(nested) == "no RawImages"


def test_type_error_for_a_nested_tensor_and_the_mode_is_kept():
    from reftr_amd.util.misc import NestedTensor
    model = _Model()
    p = Predictor(model, _post(), BatchCanvas(144, 144, 1), max_orig_size=(300, 300))
    s = _samples([(200, 300)])
    nested = dict(s, img=NestedTensor(torch.zeros(1, 3, 96, 128), torch.zeros(1, 96, 128, dtype=torch.bool)))
    for training in (True, False):
        model.train(training)
        with pytest.raises(TypeError, match="RawImages"):
            p(nested)
        with pytest.raises(TypeError, match="RawImages"):
            p({"sentence": s["sentence"]})
        assert model.training is training


def test_refusals_that_need_no_device():
    cv = BatchCanvas(144, 144, 1)
    with pytest.raises(NotImplementedError, match="GPU"):
        Predictor(_Model("cpu"), _post(), cv, max_orig_size=(300, 300))
    with pytest.raises(NotImplementedError, match="post-processor"):
        Predictor(_Model(), {"bbox": torch.nn.Identity()}, cv, max_orig_size=(300, 300))
    with pytest.raises(NotImplementedError, match="post-processor"):
        Predictor(_Model(), dict(_post(), segm=torch.nn.Identity()), cv, max_orig_size=(300, 300))
    wrapped = torch.nn.Module()
    wrapped.module = _Model()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        Predictor(wrapped, _post(), cv, max_orig_size=(300, 300))
    with pytest.raises(ValueError, match="masks=False"):
        Predictor(_Model(), _post(True), BatchCanvas(144, 144, 1, masks=True), max_orig_size=(300, 300))
