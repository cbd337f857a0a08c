"""GPU: rt_raw_stage -- raw uint8 images, pixel boxes and raw-sized target masks into the canvas buffers in one launch -- against the
chain it replaces and against the oracle.

The definition of a raw batch is BatchCanvas.pad_on_host (DeviceInputPipeline: rt_resample_u8 per pass and image, rt_img_collate_norm,
the target transforms in torch) followed by BatchCanvas.stage (rt_batch_stage); the kernel only re-does integer and correctly rounded
fp32 / fp64 arithmetic in the same order, so every gate against that chain is BIT equality (fp32 compared as int32).  Against
oracle.input_pipeline.preprocess_batch (pinned to Pillow by tests/test_input_pipeline.py) the gates are that file's: padding mask and
target masks exact, boxes 1e-6, pixels 5e-7, and the resized bytes -- recovered as round((v * std + mean) * 255) -- exact.

The kernel's tile is RT_RAW_STAGE_TILE_H x RT_RAW_STAGE_TILE_W = 32 x 64 output pixels per workgroup.  Sources of the main batch
(size 80, max_size 144): 200 x 300 -> 80 x 120 (down 2.5, 3 x 2 tiles), 300 x 200 -> 120 x 80 (4 x 2 tiles), 256 x 400 -> 80 x 125
(down 3.2), 31 x 47 -> 80 x 121 (up 2.6), 80 x 120 (identity).  The second batch into the same buffers (size 20, max_size 36) holds
outputs smaller than one tile (41 x 60 -> 20 x 29, 60 x 41 -> 29 x 20, 25 x 25 -> 20 x 20, 33 x 80 -> 15 x 36, 20 x 30 identity; none
by a whole factor, at which a checkerboard resamples to a constant): everything the first batch left must go.  Canvas
144 x 144 takes the 16-byte stores, 141 x 139 the element stores.  70 x 105 -> 120 x 180 on a 180 x 180 canvas has the axis (70 -> 120)
on which torch's fp32 `nearest` index differs from the double-precision formula.  Masks are checkerboards (x ^ y) & 1: an index off by
one flips a pixel.  Box counts 0, 1, 3 and the capacity (3)."""
import numpy as np
import pytest
import torch

from oracle import input_pipeline as IP
from reftr_amd.data import RawImages, resample
from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.data.device_input import MEAN, STD

pytestmark = pytest.mark.gpu

TAP_PAIRS = [(53, 20), (64, 128), (300, 96), (47, 47), (480, 640), (1000, 267), (375, 480), (500, 640), (427, 640), (17, 64), (1, 5)]
MAIN = dict(sizes=[(200, 300), (300, 200), (256, 400), (31, 47), (80, 120)], counts=(0, 1, 3, 3, 2), size=80, max_size=144, seed=1)
SMALL = dict(sizes=[(41, 60), (60, 41), (25, 25), (33, 80), (20, 30)], counts=(3, 0, 1, 2, 3), size=20, max_size=36, seed=2)
NEAREST = dict(sizes=[(70, 105), (105, 70)], counts=(1, 3), size=120, max_size=180, seed=3)


def make(sizes, counts, size, max_size, seed):
    """(numpy images, host targets in the raw frame, device samples, device targets)."""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    targets = []
    for (h, w), n in zip(sizes, counts):
        lo = rng.random((n, 2)) * 0.5 * np.array([w, h]); ext = (0.1 + rng.random((n, 2)) * 0.4) * np.array([w, h])
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        targets.append({"boxes": torch.from_numpy(np.concatenate([lo, lo + ext], axis=1)).float().reshape(n, 4),
                        "labels": torch.zeros(n, dtype=torch.long), "masks": torch.from_numpy(((xx ^ yy) & 1).astype(bool))[None]})
    B = len(sizes)
    s = {"img": RawImages([torch.from_numpy(i).cuda() for i in imgs], size, max_size), "sentence": torch.arange(B * 5).view(B, 5).cuda() + seed}
    t = [{k: v.cuda() for k, v in tg.items()} for tg in targets]
    return imgs, targets, s, t


@pytest.fixture(scope="module")
def batches(hip):
    return {name: make(**spec) for name, spec in (("main", MAIN), ("small", SMALL), ("nearest", NEAREST))}


@pytest.fixture(scope="module")
def oracle(batches):
    """preprocess_batch of every batch, computed once: (batch fp32 [B, 3, H, W], padding mask, targets, resized uint8 images)."""
    out = {}
    for name, spec in (("main", MAIN), ("small", SMALL), ("nearest", NEAREST)):
        imgs, targets = batches[name][:2]
        b, m, ts = IP.preprocess_batch(imgs, targets, spec["size"], spec["max_size"])
        resized = [IP.pil_bilinear_resize_u8(im, *IP.get_size_with_aspect_ratio((im.shape[1], im.shape[0]), spec["size"], spec["max_size"]))
                   for im in imgs]
        out[name] = (b, m, ts, resized)
    return out


def sentinels(cv, s):
    out = cv.alloc(s)
    out.samples["img"].tensors.fill_(float("nan"))
    out.samples["img"].mask.view(torch.uint8).fill_(0xFF)
    out.targets_static[0].fill_(float("nan")); out.targets_static[1].fill_(-1); out.targets_static[2].fill_(float("nan"))
    if out.tgt_masks is not None:
        out.tgt_masks.fill_(0xFF)
    return out


def buffers(staged):
    b = [staged.samples["img"].tensors.view(torch.int32), staged.samples["img"].mask.view(torch.uint8),
         staged.targets_static[0].view(torch.int32), staged.targets_static[1], staged.targets_static[2].view(torch.int32)]
    return b + ([staged.tgt_masks] if staged.tgt_masks is not None else [])


def same_bits(a, b):
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(buffers(a), buffers(b))):
        assert x.shape == y.shape and torch.equal(x, y), ("image", "padding mask", "boxes", "tgt_off", "num_boxes", "target masks")[i]


def against_chain(cv, out, s, t):
    """Every buffer, bit for bit, against the existing device chain: pad_on_host of the raw batch, then the existing stage."""
    ps, pt = cv.pad_on_host(s, t)
    assert tuple(ps["img"].tensors.shape[-2:]) == (cv.height, cv.width)
    want = cv.stage(ps, pt)
    same_bits(out, want)
    return want


def against_oracle(cv, out, s, ref):
    b, m, ts, resized = ref
    B, Hc, Wc = len(resized), cv.height, cv.width
    img, mask = out.samples["img"].tensors.cpu(), out.samples["img"].mask.cpu()
    want = torch.zeros(B, 3, Hc, Wc); want[:, :, :b.shape[2], :b.shape[3]] = b
    want_m = torch.ones(B, Hc, Wc, dtype=torch.bool); want_m[:, :m.shape[1], :m.shape[2]] = m
    assert torch.equal(mask, want_m)
    d = float((img - want).abs().max())
    print(f"\n[raw stage vs oracle] pixels max abs {d:.2e}")
    assert d < 5e-7
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    boxes, off, nb = (x.cpu() for x in out.targets_static)
    counts = [int(x["boxes"].shape[0]) for x in ts]
    assert off.tolist() == [sum(counts[:i]) for i in range(B + 1)] and nb.tolist() == [float(sum(counts))]
    want_boxes = torch.zeros(B * cv.boxes_per_image, 4)
    if sum(counts):
        want_boxes[:sum(counts)] = torch.cat([x["boxes"] for x in ts])
    assert float((boxes - want_boxes).abs().max()) <= 1e-6 and not boxes[sum(counts):].any()
    for i, r in enumerate(resized):
        oh, ow = r.shape[:2]
        u8 = torch.round((img[i, :, :oh, :ow].double() * std + mean) * 255).to(torch.uint8).permute(1, 2, 0).numpy()
        assert np.array_equal(u8, r), i                                               # Pillow's bytes
        assert not img[i, :, oh:].any() and not img[i, :, :, ow:].any()
        if cv.masks:
            tm = out.tgt_masks[i, 0].cpu()
            assert torch.equal(tm[:oh, :ow], ts[i]["masks"][0].to(torch.uint8)) and not tm[oh:].any() and not tm[:, ow:].any()
            assert tm[:oh, :ow].any() and not tm[:oh, :ow].all()


def test_taps_equal_the_host_taps(hip):
    """rt_resample_taps -- the device function rt_raw_stage computes its taps with -- against resample.taps: bounds, counts, every
    coefficient, zeros behind the count."""
    for n_in, n_out in TAP_PAIRS:
        b, c = resample.taps(n_in, n_out)
        for ksize in (c.shape[1], c.shape[1] + 2):
            db, dc = hip.resample_taps(n_in, n_out, ksize)
            torch.cuda.synchronize()
            assert torch.equal(db.cpu(), b), (n_in, n_out)
            assert torch.equal(dc.cpu()[:, :c.shape[1]], c) and not dc.cpu()[:, c.shape[1]:].any(), (n_in, n_out)
            assert all(not c[o, int(b[o, 1]):].any() for o in range(n_out))
    with pytest.raises(RuntimeError, match="-1"):
        hip.resample_taps(300, 96, 7)                       # 300 / 96 needs nine taps


@pytest.mark.parametrize("canvas", [(144, 144), (141, 139)])
def test_bytes_of_two_batches_into_the_same_buffers(hip, batches, oracle, canvas):
    cv = BatchCanvas(*canvas, 3, masks=True)
    _, _, s, t = batches["main"]
    assert s["img"].out_sizes() == [(80, 120), (120, 80), (80, 125), (80, 121), (80, 120)] and cv.fits(s, t)
    th, tw = hip.RAW_STAGE_TILE_H, hip.RAW_STAGE_TILE_W
    assert (th, tw) == (32, 64)
    assert sum(oh > th and ow > tw for oh, ow in s["img"].out_sizes()) >= 2       # two or more tiles in both axes
    out = sentinels(cv, s)
    assert cv.stage(s, t, out=out) is out
    against_chain(cv, out, s, t)
    against_oracle(cv, out, s, oracle["main"])
    assert torch.equal(out.samples["sentence"], s["sentence"])
    # the same bits from run to run
    again = cv.stage(s, t)
    same_bits(again, out)
    # a second, different batch into the same buffers: every output smaller than one tile
    _, _, s2, t2 = batches["small"]
    assert all(oh < th and ow < tw for oh, ow in s2["img"].out_sizes()) and s2["img"].out_sizes()[4] == (20, 30)
    cv.stage(s2, t2, out=out)
    against_chain(cv, out, s2, t2)
    against_oracle(cv, out, s2, oracle["small"])
    assert torch.equal(out.samples["sentence"], s2["sentence"])


def test_nearest_is_torch_fp32_nearest(hip, batches, oracle):
    """70 -> 120: floorf(dst * (float)(70 / 120)) and the double-precision index differ on this axis; torch's is the fp32 one."""
    f32 = [min(int(np.floor(np.float32(d) * (np.float32(70) / np.float32(120)))), 69) for d in range(120)]
    f64 = [min(int(np.floor(d * (70 / 120))), 69) for d in range(120)]
    assert f32 != f64
    cv = BatchCanvas(180, 180, 3, masks=True)
    _, _, s, t = batches["nearest"]
    assert s["img"].out_sizes() == [(120, 180), (180, 120)]
    out = sentinels(cv, s)
    cv.stage(s, t, out=out)
    against_chain(cv, out, s, t)
    against_oracle(cv, out, s, oracle["nearest"])


def test_a_canvas_without_masks_and_the_largest_batch(hip):
    """B = RT_BATCH_STAGE_MAX_B: every slot of the by-value tables is used; no target-mask buffer."""
    B = hip.BATCH_STAGE_MAX_B
    sizes = [(9 + b % 7, 11 + b % 5) for b in range(B)]
    _, _, s, t = make(sizes, tuple(b % 3 for b in range(B)), 16, 24, seed=4)
    cv = BatchCanvas(24, 32, 2)
    assert cv.fits(s, t)
    out = sentinels(cv, s)
    cv.stage(s, t, out=out)
    assert out.tgt_masks is None
    against_chain(cv, out, s, t)


def test_unsupported_scale_launches_nothing(hip):
    """400 x 600 -> 80 x 120 is a down-scale by 5: RT_ERR_UNSUPPORTED, and the pre-filled buffers stay as they were."""
    cv = BatchCanvas(144, 144, 3, masks=True)
    _, _, s, t = make([(200, 300), (400, 600)], (1, 1), 80, 144, seed=5)
    assert s["img"].out_sizes() == [(80, 120), (80, 120)] and not cv.fits(s, t)
    out = sentinels(cv, s)
    before = [b.clone() for b in buffers(out)]
    with pytest.raises(RuntimeError, match=r"rt_raw_stage failed with code -2"):
        hip.raw_stage(s["img"].images, s["img"].out_sizes(), out.samples["img"].tensors, out.samples["img"].mask,
                      [x["boxes"] for x in t], 3, *out.targets_static, MEAN, STD, mask_list=[x["masks"] for x in t], tgt_masks=out.tgt_masks)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(buffers(out), before))
    with pytest.raises(RuntimeError, match=r"code -1"):                              # a resized size beyond the canvas: RT_ERR_BADARG
        hip.raw_stage(s["img"].images[:1], [(80, 160)], out.samples["img"].tensors[:1], out.samples["img"].mask[:1],
                      [t[0]["boxes"]], 3, out.targets_static[0][:3], out.targets_static[1][:2], out.targets_static[2], MEAN, STD)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(buffers(out), before))
