"""GPU: raw batches that carry gains (RawImages.gains, the reference's colour jitter) through the batch canvas.

What a jittered raw batch MEANS is the batch whose images were replaced by reftr_amd.data.jitter.apply on the host, without gains:
rt_hsv_jitter writes those bytes into a scratch (tests/test_jitter_gpu.py) and everything behind it reads them, so every gate here is
BIT equality with the pre-jittered batch -- BatchCanvas.stage (image fp32 compared as int32, padding mask, target masks, boxes,
offsets, count), pad_on_host, resized for a batch that does not fit, and the loss vector of a replayed captured step.  The batches are
the small ones of the raw stage's own test (sizes 80 / 144: 200 x 300, 300 x 200, 256 x 400, 31 x 47, 80 x 120; sizes 20 / 36: 41 x 60,
60 x 41, 25 x 25, 33 x 80, 20 x 30), canvases 144 x 144 and 141 x 139 with masks; the step's model is the tiny one of the canvas step
tests (one bottleneck per stage, two layers each, eval mode), B = 2 on a 128 x 128 canvas."""
import numpy as np
import pytest
import torch

from reftr_amd.data import RawImages, jitter
from reftr_amd.data.canvas import BatchCanvas

pytestmark = pytest.mark.gpu

MAIN = dict(sizes=[(200, 300), (300, 200), (256, 400), (31, 47), (80, 120)], counts=(0, 1, 3, 3, 2), size=80, max_size=144, seed=1,
            gains=[(1.0, 0.5), (1.0, 1.4999), (1.0, 1.0), (0.62, 1.27), (1.0, 0.731)])
SMALL = dict(sizes=[(41, 60), (60, 41), (25, 25), (33, 80), (20, 30)], counts=(3, 0, 1, 2, 3), size=20, max_size=36, seed=2,
             gains=[(1.0, 1.269), (1.0, 0.9), (1.0, 0.55), (1.0, 1.0), (1.0, 1.45)])
MISFIT = dict(sizes=[(200, 300), (80, 100)], counts=(1, 2), size=120, max_size=180, seed=3, gains=[(1.0, 0.8), (1.0, 1.3)])


def make(sizes, counts, size, max_size, seed, gains):
    """(un-jittered samples, jittered samples, pre-jittered samples without gains, device targets, clones of the raw images)."""
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in sizes]
    t = []
    for (h, w), n in zip(sizes, counts):
        lo = rng.random((n, 2)) * 0.5 * np.array([w, h]); ext = (0.1 + rng.random((n, 2)) * 0.4) * np.array([w, h])
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        t.append({"boxes": torch.from_numpy(np.concatenate([lo, lo + ext], axis=1)).float().reshape(n, 4).cuda(),
                  "labels": torch.zeros(n, dtype=torch.long).cuda(), "masks": torch.from_numpy(((xx ^ yy) & 1).astype(bool))[None].cuda()})
    B = len(sizes)
    dev = [im.cuda() for im in imgs]
    tokens = {"sentence": torch.arange(B * 5).view(B, 5).cuda() + seed}
    plain = dict(tokens, img=RawImages(dev, size, max_size))
    jittered = dict(tokens, img=RawImages(dev, size, max_size, gains=gains))
    pre = dict(tokens, img=RawImages([jitter.apply(im, *g).cuda() for im, g in zip(imgs, gains)], size, max_size))
    return plain, jittered, pre, t, imgs


@pytest.fixture(scope="module")
def batches(hip):
    return {name: make(**spec) for name, spec in (("main", MAIN), ("small", SMALL), ("misfit", MISFIT))}


def buffers(staged):
    b = [staged.samples["img"].tensors.view(torch.int32), staged.samples["img"].mask.view(torch.uint8),
         staged.targets_static[0].view(torch.int32), staged.targets_static[1], staged.targets_static[2].view(torch.int32)]
    return b + ([staged.tgt_masks] if staged.tgt_masks is not None else [])


def same_bits(a, b):
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(buffers(a), buffers(b))):
        assert x.shape == y.shape and torch.equal(x, y), ("image", "padding mask", "boxes", "tgt_off", "num_boxes", "target masks")[i]


def same_batch(got, want):
    """(samples, targets) of pad_on_host / resized, bit for bit."""
    torch.cuda.synchronize()
    (gs, gt), (ws, wt) = got, want
    assert gs["img"].tensors.shape == ws["img"].tensors.shape
    assert torch.equal(gs["img"].tensors.view(torch.int32), ws["img"].tensors.view(torch.int32)) and torch.equal(gs["img"].mask, ws["img"].mask)
    assert torch.equal(gs["sentence"], ws["sentence"]) and len(gt) == len(wt)
    for a, b in zip(gt, wt):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                            b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


def unchanged(samples, imgs):
    torch.cuda.synchronize()
    return all(torch.equal(d.cpu(), im) for d, im in zip(samples["img"].images, imgs))


@pytest.fixture()
def launches(hip, monkeypatch):
    """The names of the library's entry points as they are called."""
    names, call = [], hip._call

    def recording(name, *args, **kw):
        names.append(name)
        return call(name, *args, **kw)
    monkeypatch.setattr(hip, "_call", recording)
    return names


@pytest.mark.parametrize("canvas", [(144, 144), (141, 139)])
def test_stage_equals_the_stage_of_the_prejittered_batch(hip, batches, launches, canvas):
    cv = BatchCanvas(*canvas, 3, masks=True)
    plain, jit, pre, t, imgs = batches["main"]
    _, jit2, pre2, t2, imgs2 = batches["small"]
    assert cv.fits(jit, t) and cv.fits(jit2, t2) and cv.key(jit) == cv.key(plain)
    # the small batch first, into fresh buffers: the scratch is made for it
    out = cv.stage(jit2, t2)
    assert launches == ["rt_hsv_jitter", "rt_raw_stage"]
    same_bits(out, cv.stage(pre2, t2))
    first = out.jitter_scratch
    need2 = sum(-(-im.numel() // 16) * 16 for im in imgs2)
    assert first is not None and first.dtype == torch.uint8 and first.numel() == need2 and first.data_ptr() % 16 == 0
    # the larger batch behind it into the same buffers: the scratch grows
    del launches[:]
    assert cv.stage(jit, t, out=out) is out
    assert launches == ["rt_hsv_jitter", "rt_raw_stage"]
    want = cv.stage(pre, t)
    same_bits(out, want)
    grown = out.jitter_scratch
    assert grown is not first and grown.numel() == sum(-(-im.numel() // 16) * 16 for im in imgs) > need2
    assert torch.equal(out.samples["sentence"], jit["sentence"])
    torch.cuda.synchronize()
    assert not torch.equal(buffers(out)[0], buffers(cv.stage(plain, t))[0])                # and the jitter did move the pixels
    # the scratch holds jitter.apply's bytes, image by image at 16-byte aligned offsets
    at = 0
    for im, g in zip(imgs, MAIN["gains"]):
        assert torch.equal(grown[at:at + im.numel()].cpu().view(im.shape), jitter.apply(im, *g))
        at += -(-im.numel() // 16) * 16
    # the small batch again: the larger scratch is reused, and nothing of the batch before is left
    cv.stage(jit2, t2, out=out)
    same_bits(out, cv.stage(pre2, t2))
    assert out.jitter_scratch is grown
    # the same bits from run to run, and the loader's tensors as they were
    same_bits(cv.stage(jit, t), want)
    assert unchanged(jit, imgs) and unchanged(jit2, imgs2)


def test_pad_on_host_and_resized_equal_the_prejittered_batch(hip, batches):
    cv = BatchCanvas(144, 144, 3, masks=True)
    _, jit, pre, t, imgs = batches["main"]
    same_batch(cv.pad_on_host(jit, t), cv.pad_on_host(pre, t))
    same_bits(cv.stage(jit, t), cv.stage(*cv.pad_on_host(jit, t)))                          # the two paths of one batch agree
    assert unchanged(jit, imgs)
    # 200 x 300 at size 120 / max_size 180 -> 120 x 180: beyond the canvas, so the batch takes `resized`
    plain, jit, pre, t, imgs = batches["misfit"]
    assert jit["img"].out_sizes() == [(120, 180), (120, 150)] and "exceeds the canvas" in cv.why_not(jit, t)
    got, want = cv.resized(jit, t), cv.resized(pre, t)
    assert tuple(got[0]["img"].tensors.shape) == (2, 3, 120, 180)
    same_batch(got, want)
    torch.cuda.synchronize()
    assert not torch.equal(got[0]["img"].tensors, cv.resized(plain, t)[0]["img"].tensors)
    assert unchanged(jit, imgs)
    # a host batch with gains: the raw bytes cross, then the same launches
    host = dict(jit, img=RawImages(imgs, MISFIT["size"], MISFIT["max_size"], gains=MISFIT["gains"]))
    same_batch(cv.resized(host, t), want)
    assert all(not im.is_cuda for im in host["img"].images)


def test_a_batch_without_gains_takes_todays_path(hip, batches, launches, monkeypatch):
    cv = BatchCanvas(144, 144, 3, masks=True)
    plain, _, _, t, imgs = batches["main"]
    assert plain["img"].gains is None
    out = cv.stage(plain, t)
    assert launches == ["rt_raw_stage"] and out.jitter_scratch is None
    ps, pt = cv.pad_on_host(plain, t)
    assert "rt_hsv_jitter" not in launches
    same_bits(out, cv.stage(ps, pt))                                                       # the parent's definition of a raw batch
    assert unchanged(plain, imgs)


# ---------------------------------------------------------------- one step: the tiny model of the canvas step tests
LAYERS = (1, 1, 1, 1)


@pytest.fixture(scope="module")
def world():
    from oracle import reftr_oracle as O
    from oracle.shapes import param_shapes
    from oracle.weights import formula_state
    ocfg = O.Cfg(enc_layers=2, dec_layers=2, bert=O.BertCfg(layers=2), resnet_layers=LAYERS)
    return {"ocfg": ocfg, "P": formula_state(param_shapes(ocfg))}


def build(world):
    from oracle import reftr_oracle as O
    from reftr_amd.models import layout as L
    from reftr_amd.models.criterion import CriterionVGMultiPhrase
    from reftr_amd.models.reftr_transformer import RefTR
    from reftr_amd.optim import FusedAdamW
    cfg = L.ModelConfig(enc_layers=2, dec_layers=2, bert=L.BertConfig(layers=2), resnet_layers=LAYERS)
    model = RefTR(cfg, device="cuda")
    model.load_state_dict(world["P"], strict=True)
    model.eval()                                         # dropout off
    crit = CriterionVGMultiPhrase(O.weight_dict(world["ocfg"]), ["boxes"])
    opt = FusedAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    return model, crit, opt


def step_batch(sizes=((72, 96), (90, 90)), counts=(3, 2), size=96, max_size=128, L=12, n_phrase=3):
    """Token fields of the oracle's synthetic batch with counts[b] valid phrases, raw uint8 images and xyxy pixel boxes."""
    from oracle.synth import make_inputs
    samples, _ = make_inputs("canvas_step", B=len(counts), H=32, W=32, L=L, n_phrase=n_phrase)
    for k in ("phrase", "phrase_mask", "phrase_pos_l", "phrase_pos_r"):
        samples[k][1:] = samples[k][0]
    for b, n in enumerate(counts):
        samples["phrase"][b, n:] = 0; samples["phrase"][b, n:, 0] = 101; samples["phrase"][b, n:, 1] = 102
        samples["phrase_mask"][b, n:] = 0; samples["phrase_mask"][b, n:, :2] = 1
        samples["phrase_pos_l"][b, n:] = 0; samples["phrase_pos_r"][b, n:] = 1
    gen = torch.Generator().manual_seed(7)
    tokens = {k: v.cuda() for k, v in samples.items() if k not in ("img", "img_mask")}
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in sizes]
    t = []
    for (h, w), n in zip(sizes, counts):
        u = torch.rand(n, 4, generator=gen)
        cx, cy, bw, bh = torch.cat([0.3 + 0.4 * u[:, :2], 0.1 + 0.4 * u[:, 2:]], dim=1).unbind(-1)
        t.append({"boxes": torch.stack([(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h], dim=-1).cuda(),
                  "labels": torch.zeros(n, dtype=torch.long).cuda()})
    return tokens, imgs, t, size, max_size


def test_replayed_step_on_a_jittered_batch(hip, world, monkeypatch):
    from reftr_amd.engine_vg import captured_train_step
    monkeypatch.setenv("REFTR_HEAD_FUSE", "0")
    cv = BatchCanvas(128, 128, 3)
    model, crit, opt = build(world)
    tokens, imgs, t, size, max_size = step_batch()
    gains = [(1.0, 0.6), (1.0, 1.4)]
    dev = [im.cuda() for im in imgs]
    plain = dict(tokens, img=RawImages(dev, size, max_size))
    jit = dict(tokens, img=RawImages(dev, size, max_size, gains=gains))
    pre = dict(tokens, img=RawImages([jitter.apply(im, *g).cuda() for im, g in zip(imgs, gains)], size, max_size))
    assert cv.fits(jit, t) and cv.key(jit) == cv.key(plain) == cv.key(pre)
    torch.cuda.synchronize()
    start = (model.store.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.step_count)

    def step(samples):
        """One captured step FROM THE SAME WEIGHTS -> [total, every loss entry]."""
        model.store.flat_p.copy_(start[0]); opt.m.copy_(start[1]); opt.v.copy_(start[2])
        opt.step_count = start[3]; opt.step_dev.fill_(start[3])
        model.mark_dirty(full=True)
        got = captured_train_step(model, crit, samples, t, opt, None, max_norm=0.1, canvas=cv)
        for c in model._captured_steps.values():
            c.flush()
        torch.cuda.synchronize()
        val = lambda v: float(v.detach()) if torch.is_tensor(v) else float(v)      # noqa: E731
        return [val(got[0])] + [val(got[2][k]) for k in sorted(got[2])]
    step(plain)                                          # (captures)
    base, a, b = step(plain), step(jit), step(pre)       # three replays of that one graph
    assert len(model._captured_steps) == 1
    cap, = model._captured_steps.values()
    assert cap.canvas is cv and cap.staged.jitter_scratch is not None
    print(f"\n[jittered step] loss {a[0]:.6f} (pre-jittered {b[0]:.6f}, un-jittered {base[0]:.6f})")
    assert all(np.isfinite(a)) and len(a) > 1
    assert a == b                                        # bit for bit
    assert a != base and a[0] != base[0]
    assert step(plain) == base                           # a replay of the un-jittered batch behind them: its own vector again
    assert all(torch.equal(d.cpu(), im) for d, im in zip(dev, imgs))
