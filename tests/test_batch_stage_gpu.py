"""GPU: rt_batch_stage against BatchCanvas.pad_on_host.  The kernel only moves bytes, so every gate is bit equality.

Destinations are pre-filled with sentinels (NaN pixels, mask bytes 7, box words -3): the buffers of a captured step hold the previous
batch, and stale pixels or mask bits from a larger predecessor are the characteristic failure -- no sentinel may survive a call.
Canvas (8, 12) takes the 16-byte image stores, canvas (7, 10) the element stores; the byte planes (padding mask, target masks) take
16-byte stores only at widths that are multiples of 16 (the production-size case).
"""
import ctypes

import pytest
import torch

from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.util.misc import NestedTensor

pytestmark = pytest.mark.gpu

BADARG, UNSUPPORTED = -1, -2


def make_batch(B, h, w, counts, mask_hw=None, seed=0, offset=0):
    """Random device batch; offset = 1 puts the image tensor one element into a larger buffer (source rows off every 16-byte line)."""
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + seed)
    n = B * 3 * h * w
    buf = torch.randn(n + 4, generator=gen).cuda()
    img = buf[offset:offset + n].view(B, 3, h, w)
    assert img.is_contiguous() and img.data_ptr() % 16 == (4 * offset) % 16
    mbuf = (torch.rand(B * h * w + 4, generator=gen) < 0.3).cuda()
    mask = mbuf[offset:offset + B * h * w].view(B, h, w)
    s = {"img": NestedTensor(img, mask), "sentence": torch.arange(B * 5).view(B, 5).cuda()}
    t = []
    for b in range(B):
        tg = {"boxes": torch.rand(counts[b], 4, generator=gen).cuda(), "labels": torch.zeros(counts[b], dtype=torch.long).cuda()}
        if mask_hw is not None:
            tg["masks"] = (torch.rand(1, *mask_hw[b], generator=gen) < 0.5).cuda()
        t.append(tg)
    return s, t


def sentinels(cv, s):
    out = cv.alloc(s)
    out.samples["img"].tensors.fill_(float("nan"))
    out.samples["img"].mask.view(torch.uint8).fill_(7)
    out.targets_static[0].fill_(-3.0); out.targets_static[1].fill_(-3); out.targets_static[2].fill_(-3.0)
    if out.tgt_masks is not None:
        out.tgt_masks.fill_(7)
    return out


def check(cv, out, s, t):
    """Every element of every destination equals pad_on_host's (bit for bit: NaN sentinels would not even compare equal)."""
    ps, pt = cv.pad_on_host(s, t)
    B = s["img"].tensors.shape[0]
    torch.cuda.synchronize()
    assert torch.equal(out.samples["img"].tensors.view(torch.int32), ps["img"].tensors.view(torch.int32))
    assert torch.equal(out.samples["img"].mask.view(torch.uint8), ps["img"].mask.view(torch.uint8))
    counts = [int(x["boxes"].shape[0]) for x in t]
    boxes, off, nb = out.targets_static
    total = sum(counts)
    want = torch.zeros(B * cv.boxes_per_image, 4, device="cuda")
    if total:
        want[:total] = torch.cat([x["boxes"] for x in t])
    assert torch.equal(boxes.view(torch.int32), want.view(torch.int32))                 # packed rows, zeroed tail
    assert off.tolist() == [sum(counts[:b]) for b in range(B + 1)]
    assert nb.tolist() == [float(total)]
    if cv.masks:
        want_m = torch.stack([x["masks"].to(torch.uint8) for x in pt])
        assert tuple(out.tgt_masks.shape) == (B, 1, cv.height, cv.width) and torch.equal(out.tgt_masks, want_m)
        assert want_m.any() and not want_m.all()


SIZES = {(8, 12): [(8, 12), (5, 7), (1, 1)], (7, 10): [(7, 10), (5, 7), (1, 1)]}


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("canvas", [(8, 12), (7, 10)])
def test_fill_every_size_no_sentinel_survives(hip, canvas, offset):
    cv = BatchCanvas(*canvas, 3, masks=True)
    for (h, w) in SIZES[canvas]:
        s, t = make_batch(3, h, w, (0, 3, 1), mask_hw=[canvas, (min(5, canvas[0]), 7), (1, 1)], offset=offset)
        out = sentinels(cv, s)
        assert cv.stage(s, t, out=out) is out
        check(cv, out, s, t)
        for k in s:
            if k != "img":
                assert torch.equal(out.samples[k], s[k])


@pytest.mark.parametrize("canvas", [(8, 12), (7, 10)])
def test_largest_then_smallest_leaves_nothing_behind(hip, canvas):
    """The stale-data case: the same buffers first hold a canvas-sized batch with every box slot and a full mask, then a 1 x 1 one."""
    cv = BatchCanvas(*canvas, 3, masks=True)
    big = make_batch(3, *canvas, (3, 3, 3), mask_hw=[canvas] * 3, seed=1)
    small = make_batch(3, 1, 1, (0, 0, 0), mask_hw=[(1, 1)] * 3, seed=2)
    out = sentinels(cv, big[0])
    cv.stage(*big, out=out)
    check(cv, out, *big)
    cv.stage(*small, out=out)
    fresh = cv.stage(*small)
    torch.cuda.synchronize()
    assert torch.equal(out.samples["img"].tensors, fresh.samples["img"].tensors) and not out.samples["img"].tensors[:, :, 1:, 1:].any()
    assert torch.equal(out.samples["img"].mask, fresh.samples["img"].mask)
    assert all(torch.equal(a, b) for a, b in zip(out.targets_static, fresh.targets_static))
    assert torch.equal(out.tgt_masks, fresh.tgt_masks)
    # and the same bits from run to run
    again = cv.stage(*small)
    assert torch.equal(again.samples["img"].tensors, fresh.samples["img"].tensors)


def test_box_counts_offsets_and_tail(hip):
    cv = BatchCanvas(8, 12, 3)
    s, t = make_batch(3, 5, 7, (0, 3, 1))
    out = sentinels(cv, s)
    cv.stage(s, t, out=out)
    check(cv, out, s, t)
    boxes, off, nb = out.targets_static
    assert off.tolist() == [0, 0, 3, 4] and nb.item() == 4.0
    assert torch.equal(boxes[:3], t[1]["boxes"]) and torch.equal(boxes[3], t[2]["boxes"][0]) and not boxes[4:].any()
    s0, t0 = make_batch(3, 5, 7, (0, 0, 0))
    cv.stage(s0, t0, out=out)
    check(cv, out, s0, t0)
    assert off.tolist() == [0, 0, 0, 0] and nb.item() == 0.0 and not boxes.any()


@pytest.mark.parametrize("src", [(427, 640), (640, 427)])
def test_production_size(hip, src):
    """B = 8 at 3 x 640 x 640: 2.46 M 16-byte image units over 2048 workgroups -- the grid-stride loop runs more than four rounds,
    and the byte planes take their 16-byte stores (640 % 16 == 0).  A 427-wide source has no aligned row but the first."""
    cv = BatchCanvas(640, 640, 1, masks=True)
    s, t = make_batch(8, *src, (1,) * 8, mask_hw=[src] * 8)
    out = sentinels(cv, s)
    cv.stage(s, t, out=out)
    check(cv, out, s, t)


def test_kernel_refuses_bad_arguments(hip):
    H = hip
    L = H.lib()
    B, cap, Hc, Wc, hs, ws = 3, 3, 8, 12, 5, 7
    src = torch.ones(B, 3, hs, ws, device="cuda"); smask = torch.zeros(B, hs, ws, dtype=torch.uint8, device="cuda")
    img = torch.full((B, 3, Hc, Wc), 5.0, device="cuda"); mask = torch.full((B, Hc, Wc), 7, dtype=torch.uint8, device="cuda")
    boxes = torch.full((B * cap, 4), -3.0, device="cuda"); off = torch.full((B + 1,), -3, dtype=torch.int32, device="cuda")
    nb = torch.full((1,), -3.0, device="cuda"); tmask = torch.full((B, 1, Hc, Wc), 7, dtype=torch.uint8, device="cuda")
    bsrc = [torch.rand(3, 4, device="cuda") for _ in range(B)]
    msrc = [torch.ones(1, 4, 4, dtype=torch.uint8, device="cuda") for _ in range(B)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    null = ctypes.c_void_p(0)
    vp = lambda ts, n=B: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    iv = lambda xs: (ctypes.c_int32 * len(xs))(*xs)                       # noqa: E731
    good = dict(src=p(src), smask=p(smask), B=B, hs=hs, ws=ws, img=p(img), mask=p(mask), Hc=Hc, Wc=Wc, bp=vp(bsrc), bn=iv([0, 3, 1]),
                cap=cap, boxes=p(boxes), off=p(off), nb=p(nb), tp=vp(msrc), thw=iv([4, 4] * B), tmask=p(tmask))

    def call(**kw):
        a = dict(good, **kw)
        return L.rt_batch_stage(a["src"], a["smask"], a["B"], a["hs"], a["ws"], a["img"], a["mask"], a["Hc"], a["Wc"], a["bp"], a["bn"],
                                a["cap"], a["boxes"], a["off"], a["nb"], a["tp"], a["thw"], a["tmask"], null)

    for name in ("src", "smask", "img", "mask", "boxes", "off", "nb"):                  # a null required pointer
        assert call(**{name: null}) == BADARG, name
    assert call(bp=None) == BADARG and call(bn=None) == BADARG
    assert call(tp=None) == BADARG and call(thw=None) == BADARG and call(tmask=null) == BADARG      # target masks: all or none
    for name in ("B", "hs", "ws", "Hc", "Wc", "cap"):                                   # a non-positive size
        assert call(**{name: 0}) == BADARG and call(**{name: -2}) == BADARG, name
    assert call(hs=Hc + 1) == BADARG and call(ws=Wc + 1) == BADARG                      # a source larger than the canvas
    assert call(thw=iv([4, 4, Hc + 1, 4, 4, 4])) == BADARG and call(thw=iv([4, 4, 4, Wc + 1, 4, 4])) == BADARG
    assert call(thw=iv([4, 4, 0, 4, 4, 4])) == BADARG
    assert call(bn=iv([0, cap + 1, 1])) == BADARG and call(bn=iv([0, -1, 1])) == BADARG  # a count above the capacity
    assert call(bp=(ctypes.c_void_p * B)(bsrc[0].data_ptr(), None, bsrc[2].data_ptr())) == BADARG   # boxes counted but not given
    nmax = H.BATCH_STAGE_MAX_B
    assert nmax >= 64
    many = dict(B=nmax + 1, bp=vp((bsrc * (nmax + 1))[:nmax + 1], nmax + 1), bn=iv([0] * (nmax + 1)),
                tp=vp((msrc * (nmax + 1))[:nmax + 1], nmax + 1), thw=iv([4, 4] * (nmax + 1)))
    assert call(**many) == UNSUPPORTED                                                  # above what the argument block holds
    torch.cuda.synchronize()
    assert (img == 5).all() and (mask == 7).all() and (boxes == -3).all() and (off == -3).all() and (nb == -3).all() and (tmask == 7).all()
    assert call() == 0                                                                  # ... and the good call is one
    torch.cuda.synchronize()
    assert (mask != 7).all() and (tmask != 7).all() and off.tolist() == [0, 0, 3, 4] and nb.item() == 4.0


def test_largest_batch_the_argument_block_holds(hip):
    """B = RT_BATCH_STAGE_MAX_B: every slot of the by-value tables is used."""
    B = hip.BATCH_STAGE_MAX_B
    cv = BatchCanvas(8, 12, 2, masks=True)
    s, t = make_batch(B, 5, 7, tuple(b % 3 for b in range(B)), mask_hw=[(1 + b % 8, 1 + b % 12) for b in range(B)])
    out = sentinels(cv, s)
    cv.stage(s, t, out=out)
    check(cv, out, s, t)
