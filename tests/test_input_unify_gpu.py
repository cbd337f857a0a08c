"""GPU: the shared definitions of the image side -- rt_weight_prep through the tile body of rt_weight_prep_batched, rt_raw_stage's choice
of a unit's width per destination pointer (csrc/rt_stage.h), and the box tails of rt_batch_stage and rt_raw_stage against each other.
Every gate is bit equality."""
import pytest
import torch

from reftr_amd.data.canvas import BatchCanvas
from reftr_amd.util.misc import NestedTensor
from test_raw_stage_gpu import SMALL, buffers, make, same_bits

pytestmark = pytest.mark.gpu

# (N, T, C, scaled): both vector paths | both element paths | transposed vector, direct element | direct vector, transposed element |
# ragged with several taps | 3 x 2 ragged tiles
PREP = [(24, 9, 16, True), (100, 1, 70, False), (72, 1, 100, False), (100, 1, 72, False), (33, 4, 33, True), (130, 1, 65, False)]
SENTINEL = -3.0


def off_by_one(shape, dtype, fill):
    """(buffer, view): a contiguous `shape` view that starts one element into a larger buffer filled with `fill`."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 16,), fill, dtype=dtype, device="cuda")
    return buf, buf[1:1 + n].view(shape)


def untouched(buf, n, fill):
    """The elements before and behind the view of off_by_one still hold `fill` (NaN compares as NaN)."""
    rest = torch.cat([buf[:1], buf[1 + n:]])
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


@pytest.mark.parametrize("N,T,C,scaled", PREP)
def test_single_weight_prep_runs_the_tile_body(hip, N, T, C, scaled):
    g = torch.Generator().manual_seed(100 * N + C)
    src = torch.randn(N, T, C, generator=g)
    sc = (torch.rand(N, generator=g) + 0.5) if scaled else None
    ref = (src * sc.view(-1, 1, 1) if scaled else src).bfloat16()
    ref_t = ref.permute(2, 1, 0).contiguous()
    src_c, sc_c = src.cuda(), (sc.cuda() if scaled else None)

    def fresh(misaligned):
        if misaligned:
            return off_by_one((N, T, C), torch.bfloat16, SENTINEL), off_by_one((C, T, N), torch.bfloat16, SENTINEL)
        d, dt = torch.full((N, T, C), SENTINEL, dtype=torch.bfloat16, device="cuda"), torch.full((C, T, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
        return (d, d), (dt, dt)

    for want_dst, want_t, misaligned in ((True, False, False), (False, True, False), (True, True, False), (True, True, True)):
        for single in (True, False):
            (buf, dst), (buf_t, dst_t) = fresh(misaligned)
            kw = dict(scale=sc_c, dst=dst if want_dst else None, dst_t=dst_t if want_t else None)
            if single:
                hip.weight_prep(src_c, N, T, C, **kw)
            else:
                batch = hip.WeightPrepBatch("cuda")
                batch.add(src_c, N, T, C, **kw)
                batch.run()
            torch.cuda.synchronize()
            what = (N, T, C, want_dst, want_t, misaligned, "single" if single else "one-job batch")
            assert torch.equal(dst.cpu(), ref) if want_dst else bool((dst == SENTINEL).all()), what
            assert torch.equal(dst_t.cpu(), ref_t) if want_t else bool((dst_t == SENTINEL).all()), what
            if misaligned:
                assert dst.data_ptr() % 16 == 2 and dst_t.data_ptr() % 16 == 2
                assert untouched(buf, N * T * C, SENTINEL) and untouched(buf_t, N * T * C, SENTINEL), what


@pytest.fixture(scope="module")
def small(hip):
    """The SMALL batch of test_raw_stage_gpu.py on a 144 x 144 canvas with masks, and its staging into aligned buffers."""
    cv = BatchCanvas(144, 144, 3, masks=True)
    _, _, s, t = make(**SMALL)
    return cv, s, t, cv.stage(s, t)


@pytest.mark.parametrize("which", ["img", "mask", "tgt_masks"])
def test_raw_stage_with_one_misaligned_destination(hip, small, which):
    """The staged buffer `which` is a view one element into a larger sentinel-filled tensor (one float, one byte): the width of its
    units follows from its own pointer, and every buffer equals the aligned staging."""
    cv, s, t, want = small
    B, Hc, Wc = len(s["img"]), cv.height, cv.width
    out = cv.alloc(s)
    fill = {"img": float("nan"), "mask": 0xFF, "tgt_masks": 0xFF}[which]
    shape = {"img": (B, 3, Hc, Wc), "mask": (B, Hc, Wc), "tgt_masks": (B, 1, Hc, Wc)}[which]
    buf, view = off_by_one(shape, torch.float32 if which == "img" else torch.uint8, fill)
    img, mask = out.samples["img"].tensors, out.samples["img"].mask
    if which == "img":
        img = view
    elif which == "mask":
        mask = view.view(torch.bool)
    else:
        out.tgt_masks = view
    out.samples["img"] = NestedTensor(img, mask)
    assert view.data_ptr() % 16 == (4 if which == "img" else 1)
    assert sum(b.data_ptr() % 16 != 0 for b in (img, mask, out.tgt_masks)) == 1
    assert cv.stage(s, t, out=out) is out
    same_bits(out, want)
    assert untouched(buf, view.numel(), fill)


def test_box_tails_of_batch_stage_and_raw_stage_agree(hip):
    """Raw images that already have their output size (rw = rh = 1), box counts 0, 1, the capacity and 2: the raw staging and the
    staging of the pad_on_host NestedTensor batch write the same box tail."""
    sizes, counts = [(20, 30), (20, 25), (30, 20), (20, 20)], (0, 1, 3, 2)
    _, _, s, t = make(sizes, counts, 20, 36, seed=6)
    assert s["img"].out_sizes() == sizes
    cv = BatchCanvas(32, 48, 3)
    raw = cv.stage(s, t)
    nested = cv.stage(*cv.pad_on_host(s, t))
    torch.cuda.synchronize()
    (boxes, off, nb), (boxes_n, off_n, nb_n) = raw.targets_static, nested.targets_static
    assert off.tolist() == [0, 0, 1, 4, 6] and nb.tolist() == [6.0]
    assert torch.equal(off, off_n) and torch.equal(nb, nb_n)
    assert torch.equal(boxes.view(torch.int32), boxes_n.view(torch.int32))
    assert boxes[:6].abs().min() > 0 and not boxes[6:].any()
    same_bits(raw, nested)
