"""CPU: the colour jitter's definition (reftr_amd/data/jitter.py), the gains a raw batch carries, rt_hsv_jitter's row of the binding
with every argument check that returns before a launch, and the two refusals.  Nothing here launches.

The definition is held three ways: to the check values of the text it restates; to properties over ALL 256^3 colours (one 4096 x 4096
image); and to an independent numpy transcription of the same text (`emulate`), which also plays the WRONG kernels -- each switch of
it is one way a device kernel can go wrong, and each must change at least one colour of the exhaustive set, or the GPU test that
compares the kernel with `apply` on that set could not tell it apart.

One of the listed wrong kernels is not wrong: tables rounded half UP.  None of the 2 x 255 quotients (255 << 12) / i and (180 << 12) /
(6 i) lies on a tie -- 2 * 255 * 2^12 / i and 2 * 30 * 2^12 / i are never odd integers for i < 256, their powers of two being 2^13 --
so half-up and half-to-even give the same tables and the same bytes everywhere; test_half_up_tables_are_the_same_tables holds that,
and the table rounding that CAN go wrong (truncation, what a bare (int) cast does) is the `trunc_tables` switch."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from reftr_amd import Predictor, evaluate_raw, hip
from reftr_amd.data import RawImages, jitter, raw_collate
from reftr_amd.data.canvas import BatchCanvas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = -1, -2
F = np.float32
COLOURS = [(200, 100, 50), (12, 200, 180), (1, 2, 3), (130, 7, 255)]
SECT = np.array([(1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0)], dtype=np.int8)          # (b, g, r)


# ---------------------------------------------------------------- the numpy transcription, with its wrong-kernel switches
def emu_tables(rounding="even"):
    i = np.arange(1, 256, dtype=np.float64)
    rnd = {"even": np.rint, "half_up": lambda x: np.floor(x + 0.5), "trunc": np.floor}[rounding]
    sdiv, hdiv = np.zeros(256, np.int32), np.zeros(256, np.int32)
    sdiv[1:] = rnd((255 << 12) / (1.0 * i))
    hdiv[1:] = rnd((180 << 12) / (6.0 * i))
    return sdiv, hdiv


def emu_rgb_to_hsv(rgb, tables=None, div=False):
    """rgb uint8 [N, 3] -> h, s, v int32 [N]; `div`: the shift of the hue product replaced by C's division (toward zero)."""
    sdiv, hdiv = tables if tables is not None else emu_tables()
    r, g, b = (rgb[:, c].astype(np.int32) for c in range(3))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = (d * sdiv[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    x = h0 * hdiv[d] + 2048
    h = (np.abs(x) // 4096) * np.sign(x) if div else x >> 12
    return np.where(h < 0, h + 180, h), s, v


def emu_gain(x, gain, clip=True):
    g = F(gain)
    y = x.astype(F) * g
    if g > 1 and clip:
        y = np.minimum(np.maximum(y, F(0)), F(255))
    return y.astype(np.int32).astype(np.uint8).astype(np.int32)          # (uint8)(int)y: without the clip it wraps


def emu_hsv_to_rgb(h, s, v, fma=False, trunc=False):
    """`fma`: the two products a compiler can contract, 1 - sf * f and 1 - sf * (1 - f), rounded once (the product is exact in
    double); `trunc`: truncation in place of rintf at the output."""
    one = F(1)
    hf, sf, vf = h.astype(F) * (F(6) / F(180)), s.astype(F) * (one / F(255)), v.astype(F) * (one / F(255))
    fl = np.floor(hf)
    sector, f = fl.astype(np.int32), hf - fl
    outside = (sector < 0) | (sector > 5)
    sector[outside], f[outside] = 0, 0
    if fma:
        nfma = lambda a, b: (1.0 - a.astype(np.float64) * b.astype(np.float64)).astype(F)
        i2, i3 = nfma(sf, f), nfma(sf, one - f)
    else:
        i2, i3 = one - sf * f, one - sf * (one - f)
    tab = [vf, vf * (one - sf), vf * i2, vf * i3]
    out = np.empty((h.shape[0], 3), np.uint8)
    for ch in range(3):                                                  # SECT's columns are b, g, r
        c = np.where(s == 0, vf, np.choose(SECT[sector, ch], tab))
        x = c * F(255)
        out[:, 2 - ch] = np.clip(np.trunc(x) if trunc else np.rint(x), 0, 255).astype(np.uint8)
    return out


def emulate(rgb, s_gain, v_gain, **kw):
    h, s, v = emu_rgb_to_hsv(rgb)
    return emu_hsv_to_rgb(h, emu_gain(s, s_gain), emu_gain(v, v_gain), **kw)


# ---------------------------------------------------------------- all 256^3 colours, computed once and left unchanged
@pytest.fixture(scope="module")
def everything():
    i = torch.arange(1 << 24, dtype=torch.int32)
    img = torch.stack([i >> 16, (i >> 8) & 255, i & 255], dim=-1).to(torch.uint8).view(4096, 4096, 3)
    flat = img.view(-1, 3).numpy()
    cache = {}

    def applied(s_gain, v_gain):
        if (s_gain, v_gain) not in cache:
            cache[s_gain, v_gain] = jitter.apply(img, s_gain, v_gain).view(-1, 3).numpy()
        return cache[s_gain, v_gain]
    return SimpleNamespace(img=img, flat=flat, applied=applied, hsv=emu_rgb_to_hsv(flat))


def differing(a, b):
    return int((a != b).any(axis=1).sum())


# ---------------------------------------------------------------- values
def test_tables_and_conversion_check_values():
    sdiv, hdiv = jitter.tables()
    assert sdiv.dtype == torch.int32 and tuple(sdiv.shape) == (256,) and tuple(hdiv.shape) == (256,)
    assert int(sdiv[0]) == 0 and int(hdiv[0]) == 0
    assert sdiv[[1, 3, 255]].tolist() == [1044480, 348160, 4096] and hdiv[[1, 7, 255]].tolist() == [122880, 17554, 482]
    assert np.array_equal(sdiv.numpy(), emu_tables()[0]) and np.array_equal(hdiv.numpy(), emu_tables()[1])
    px = torch.tensor([(200, 100, 50), (12, 200, 180), (130, 7, 255), (1, 2, 3)], dtype=torch.uint8)
    h, s, v = jitter.rgb_to_hsv(px)
    assert list(zip(h.tolist(), s.tolist(), v.tolist())) == [(10, 191, 200), (87, 240, 200), (135, 248, 255), (105, 170, 3)]
    assert jitter.hsv_to_rgb(h, s, v).dtype == torch.uint8


@pytest.mark.parametrize("gains,want", [
    ((1, 1), [(200, 100, 50), (12, 200, 181), (1, 2, 3), (131, 7, 255)]),
    ((1, 0.5), [(100, 50, 25), (6, 100, 91), (0, 1, 1), (65, 3, 127)]),
    ((1, 1.5), [(255, 128, 64), (15, 255, 231), (1, 3, 4), (131, 7, 255)]),
    ((0.62, 1.27), [(254, 176, 136), (107, 254, 239), (2, 2, 3), (178, 102, 255)])])
def test_gain_check_values(gains, want):
    img = torch.tensor(COLOURS, dtype=torch.uint8).view(2, 2, 3)
    got = jitter.apply(img, *gains)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 2, 3)
    assert [tuple(p) for p in got.view(-1, 3).tolist()] == want
    assert [tuple(p) for p in emulate(img.view(-1, 3).numpy(), *gains).tolist()] == want


# ---------------------------------------------------------------- properties over every colour
def test_hue_range_and_round_trip_over_all_colours(everything):
    h, s, v = jitter.rgb_to_hsv(everything.img)
    assert int(h.min()) == 0 and int(h.max()) < 180 and int(s.min()) == 0 and int(s.max()) == 255 and int(v.max()) == 255
    assert all(np.array_equal(a.view(-1).numpy(), b) for a, b in zip((h, s, v), everything.hsv))
    out = everything.applied(1, 1)
    moved = np.abs(out.astype(np.int16) - everything.flat.astype(np.int16))
    changed = differing(out, everything.flat) / float(1 << 24)
    print(f"\n[jitter] gains (1, 1): {100 * changed:.2f} % of the colours change, by at most {int(moved.max())} levels")
    assert int(moved.max()) <= 5 and round(changed, 3) == 0.689


@pytest.mark.parametrize("gains", [(1, 1), (1, 0.5), (1, 1.4999), (0.62, 1.27), (0, 0), (1.5, 1.5)])
def test_greys_stay_grey(gains):
    grey = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).expand(16, 16, 3).contiguous()
    out = jitter.apply(grey, *gains)
    assert torch.equal(out[..., 0], out[..., 1]) and torch.equal(out[..., 1], out[..., 2])
    if gains[1] == 1:
        assert torch.equal(out, grey)


@pytest.mark.parametrize("gains", [(1, 1), (0.62, 1.27)])
def test_the_transcription_is_the_definition(everything, gains):
    h, s, v = everything.hsv
    assert differing(emu_hsv_to_rgb(h, emu_gain(s, gains[0]), emu_gain(v, gains[1])), everything.applied(*gains)) == 0


# ---------------------------------------------------------------- the exhaustive set tells wrong kernels apart
@pytest.mark.parametrize("v_gain", [1.0, 0.731, 1.269])
def test_contracted_products_differ(everything, v_gain):
    h, s, v = everything.hsv
    n = differing(emu_hsv_to_rgb(h, s, emu_gain(v, v_gain), fma=True), everything.applied(1, v_gain))
    print(f"\n[jitter] FMA-contracted products, v_gain {v_gain}: {n} of 2^24 colours differ")
    assert n > 0


def test_truncated_output_differs(everything):
    h, s, v = everything.hsv
    assert differing(emu_hsv_to_rgb(h, s, v, trunc=True), everything.applied(1, 1)) > 0


def test_missing_clip_differs(everything):
    h, s, v = everything.hsv
    assert differing(emu_hsv_to_rgb(h, s, emu_gain(v, 1.269, clip=False)), everything.applied(1, 1.269)) > 0
    assert differing(emu_hsv_to_rgb(h, emu_gain(s, 1.27, clip=False), v), everything.applied(1.27, 1)) > 0


def test_division_for_the_shift_differs(everything):
    _, s, v = everything.hsv
    h = emu_rgb_to_hsv(everything.flat, div=True)[0]
    assert int((h != everything.hsv[0]).sum()) > 0
    assert differing(emu_hsv_to_rgb(h, s, v), everything.applied(1, 1)) > 0


def test_truncated_tables_differ(everything):
    h, s, v = emu_rgb_to_hsv(everything.flat, tables=emu_tables("trunc"))
    assert differing(emu_hsv_to_rgb(h, s, v), everything.applied(1, 1)) > 0


def test_half_up_tables_are_the_same_tables():
    """(see the module docstring) no quotient lies on a tie, so this `wrong` kernel computes the definition's tables."""
    i = np.arange(1, 256, dtype=np.float64)
    for q in ((255 << 12) / (1.0 * i), (180 << 12) / (6.0 * i)):
        frac = q - np.floor(q)
        assert float(np.abs(frac - 0.5).min()) > 1e-3
    for a, b in zip(emu_tables("half_up"), emu_tables("even")):
        assert np.array_equal(a, b)
    assert any(not np.array_equal(a, b) for a, b in zip(emu_tables("trunc"), emu_tables("even")))


# ---------------------------------------------------------------- plumbing
def item(h, w, n_boxes=1, L=5):
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8)
    fields = {"sentence": torch.arange(L), "sentence_mask": torch.ones(L, dtype=torch.bool)}
    return img, fields, {"boxes": torch.rand(n_boxes, 4) * torch.tensor([w, h, w, h]), "labels": torch.zeros(n_boxes, dtype=torch.long)}


def test_draw_gains_consumes_two_draws_per_image_in_order():
    random.seed(11)
    draws = [random.random() for _ in range(7)]
    random.seed(11)
    gains = jitter.draw_gains(3)
    assert gains == [(1.0, (draws[2 * k + 1] * 2 - 1) * 0.5 + 1) for k in range(3)]
    assert random.random() == draws[6]                                    # six draws consumed, no more
    assert all(0.5 <= v <= 1.5 for _, v in gains)
    own = random.Random(5)
    twin = random.Random(5)
    twin.random()
    assert jitter.draw_gains(1, rng=own) == [(1.0, (twin.random() * 2 - 1) * 0.5 + 1)]
    assert jitter.draw_gains(0) == []


def test_collate_and_raw_images_carry_the_gains():
    items = [item(20, 30), item(31, 17), item(8, 8)]
    s, _ = raw_collate(80, 144)(items)
    assert s["img"].gains is None                                         # the default: today's batch
    assert raw_collate(80, 144, jitter=False)(items)[0]["img"].gains is None and RawImages([items[0][0]], 80).gains is None
    random.seed(3)
    s, _ = raw_collate(80, 144, jitter=True)(items)
    random.seed(3)
    img = s["img"]
    assert img.gains == jitter.draw_gains(3) and img.well_formed() and all(torch.equal(a, b[0]) for a, b in zip(img.images, items))
    moved, pinned_like = img.to("cpu", non_blocking=True), RawImages(img.images, 80, 144, gains=img.gains)
    assert moved.gains == img.gains and moved.out_sizes() == img.out_sizes() and pinned_like.gains == img.gains
    if torch.cuda.is_available():
        assert img.pin_memory().gains == img.gains
    else:                                                                  # no device to pin for: the method's own lines on a stand-in
        class Pinned(torch.Tensor):
            def pin_memory(self):
                return self
        twin = RawImages([im.as_subclass(Pinned) for im in img.images], 80, 144, gains=img.gains).pin_memory()
        assert twin.gains == img.gains and (twin.size, twin.max_size) == (80, 144)
    from reftr_amd.engine_vg import _to_device
    assert _to_device(s, [], torch.device("cpu"))[0]["img"].gains == img.gains
    moved.record_stream(None)
    # host floats whatever came in
    assert RawImages(img.images, 80, gains=[(np.float32(1), torch.tensor(0.5))] * 3).gains == [(1.0, 0.5)] * 3


def test_well_formed_and_why_not_reject_bad_gains():
    images = [torch.zeros(20, 30, 3, dtype=torch.uint8), torch.zeros(30, 20, 3, dtype=torch.uint8)]
    t = [{"boxes": torch.zeros(1, 4)}, {"boxes": torch.zeros(0, 4)}]
    cv = BatchCanvas(144, 144, 3)
    assert RawImages(images, 80, 144, gains=[(1.0, 0.5), (0.0, 1.5)]).well_formed()
    for gains in ([(1.0, 1.0)], [(1.0, 1.0)] * 3, [(1.0, -0.1), (1.0, 1.0)], [(1.0, 1.0), (float("nan"), 1.0)],
                  [(1.0, float("inf")), (1.0, 1.0)]):
        img = RawImages(images, 80, 144, gains=gains)
        assert not img.well_formed(), gains
        assert "gains" in cv.why_not({"img": img}, t)
    assert cv.why_not({"img": RawImages(images, 80, 144, gains=[(1.0, 0.7), (1.0, 1.2)])}, t) is None
    # a capture's key does not know about gains
    assert cv.key({"img": RawImages(images, 80, 144, gains=[(1.0, 0.7), (1.0, 1.2)])}) == cv.key({"img": RawImages(images, 80, 144)})


# ---------------------------------------------------------------- the binding
def test_abi_row_and_argument_block():
    header = open(os.path.join(ROOT, "include", "reftr_hip.h")).read()
    assert hip.ABI_VERSION == 39                                          # purely additive
    assert re.search(r"\bint rt_hsv_jitter\(const rt_hsv_jitter_args\* a, rt_stream_t stream\);", header)
    res, args = hip._SIGNATURES["rt_hsv_jitter"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(hip.HsvJitterArgs), ctypes.c_void_p]
    assert hip.STRUCTS["rt_hsv_jitter_args"] is hip.HsvJitterArgs
    # everything rides by value: the struct is the kernel's only argument (no scalar words beside it) and stays under the launch's 4 KB
    n = hip.BATCH_STAGE_MAX_B
    assert ctypes.sizeof(hip.HsvJitterArgs) + 0 * 4 <= 4096 and ctypes.sizeof(hip.HsvJitterArgs) == 8 + (8 + 8 + 4 * 4) * n
    assert all(getattr(hip.HsvJitterArgs, f).size == n * (8 if f in ("src", "dst") else 4) for f in ("src", "dst", "h", "w", "s_gain", "v_gain"))
    a = hip._desc(hip.HsvJitterArgs, B=2, h=[5, 7], v_gain=[0.5], src=[None, None])
    assert list(a.h)[:3] == [5, 7, 0] and a.v_gain[0] == 0.5 and a.s_gain[0] == 0.0 and a.dst[0] is None


def test_argument_checks_return_before_any_launch():
    """Every RT_ERR_BADARG / RT_ERR_UNSUPPORTED case: decided on the host from the argument block alone (the pointers are never
    followed), so no device is needed."""
    L, n = hip.lib(), hip.BATCH_STAGE_MAX_B
    FAKE = 0x1000

    def call(B=2, src=(FAKE, FAKE), dst=(FAKE, FAKE + 4096), h=(3, 5), w=(4, 6), s_gain=(1.0, 1.0), v_gain=(0.7, 1.3)):
        a = hip.HsvJitterArgs(B=B, src=(ctypes.c_void_p * n)(*src), dst=(ctypes.c_void_p * n)(*dst), h=(ctypes.c_int32 * n)(*h),
                              w=(ctypes.c_int32 * n)(*w), s_gain=(ctypes.c_float * n)(*s_gain), v_gain=(ctypes.c_float * n)(*v_gain))
        return L.rt_hsv_jitter(ctypes.byref(a), None)
    assert L.rt_hsv_jitter(None, None) == BAD
    for kw in (dict(B=0), dict(B=-1), dict(src=(FAKE, None)), dict(dst=(None, FAKE)), dict(h=(0, 5)), dict(h=(3, -1)), dict(w=(4, 0)),
               dict(w=(-4, 6)), dict(v_gain=(0.7, -0.1)), dict(s_gain=(-0.1, 1.0)), dict(v_gain=(float("nan"), 1.0)),
               dict(s_gain=(1.0, float("nan"))), dict(v_gain=(1.0, float("inf"))), dict(s_gain=(float("inf"), 1.0))):
        assert call(**kw) == BAD, kw
    assert call(B=n + 1) == UNSUPPORTED
    assert call(h=(3, 1 << 15), w=(4, 21846)) == UNSUPPORTED              # 3 * 32768 * 21846 = 2^31 + 2^16
    assert call(h=(3, 1 << 16), w=(4, 1 << 16)) == UNSUPPORTED            # h * w itself beyond 32 bits


# ---------------------------------------------------------------- the refusals
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


def _jittered_batch():
    random.seed(1)
    return raw_collate(80, 144, jitter=True)([item(200, 300), item(300, 200)])


def test_evaluate_raw_refuses_gains():
    model, crit = _Model(), _Criterion()
    model.train(); crit.train()
    with pytest.raises(ValueError, match="gains"):
        evaluate_raw(model, crit, _post(), [_jittered_batch()], torch.device("cuda"), BatchCanvas(144, 144, 3))
    assert model.training and crit.training                               # nothing was touched


def test_predictor_refuses_gains():
    model = _Model()
    s, _ = _jittered_batch()
    p = Predictor(model, _post(), BatchCanvas(144, 144, 1), max_orig_size=(300, 300))
    for training in (True, False):
        model.train(training)
        with pytest.raises(ValueError, match="gains"):
            p(s)
        assert model.training is training and not p.steps
