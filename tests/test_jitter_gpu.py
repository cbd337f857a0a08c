"""GPU: rt_hsv_jitter -- the colour jitter of a raw batch in one launch -- against its definition, reftr_amd.data.jitter.apply (plain torch
on the CPU, held by tests/test_jitter_cpu.py).  The kernel re-does integer and correctly rounded fp32 / fp64 arithmetic in the same
order, so every gate is BYTE equality, zero differing elements.

All 256^3 colours (one 4096 x 4096 image) under four pairs of gains: the CPU file shows that this set tells apart a kernel whose fp32
products are contracted, whose output truncates, whose clip is missing or whose hue shift is a division.  Addressing: a thread's unit
is 16 consecutive pixels of the flat image, 48 bytes, moved as three 16-byte words where the unit lies wholly inside the image and
both bases are 16-byte aligned, byte by byte otherwise; the batch below has images smaller than a unit (1 x 1, 3 x 5), images whose
last unit is partial behind many whole ones (31 x 47 = 91 units + 1 pixel, 37 x 53 = 122 + 9), none with 3 * w a multiple of 16 but
64 x 64 (256 whole units), aligned and odd bases on either side, and 16 poisoned guard bytes around every destination."""
import ctypes

import pytest
import torch

from reftr_amd.data import jitter

pytestmark = pytest.mark.gpu

BAD, UNSUPPORTED = -1, -2
SIZES_A = [(1, 1), (3, 5), (31, 47), (37, 53), (64, 64)]
GAINS_A = [(1.0, 1.0), (1.0, 0.5), (0.62, 1.27), (1.0, 1.4999), (1.3, 0.731)]
SIZES_B = [(2, 7), (16, 16), (5, 3), (48, 33), (1, 17)]
GAINS_B = [(1.0, 1.269), (0.0, 1.0), (1.0, 0.0), (1.0, 0.9), (1.5, 1.5)]


@pytest.fixture(scope="module")
def all_colours(hip):
    i = torch.arange(1 << 24, dtype=torch.int32)
    img = torch.stack([i >> 16, (i >> 8) & 255, i & 255], dim=-1).to(torch.uint8).view(4096, 4096, 3)
    return img, img.cuda()


def host_images(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in sizes]


def carve(arena, sizes, align, first=16, guard=16):
    """Views [h, w, 3] into the byte arena with at least `guard` bytes in front of, between and behind them; align[k]: None (where it
    falls), 16 (the next 16-byte aligned offset) or 1 (the next ODD offset).  Returns (views, [(offset, bytes)])."""
    views, spans, at = [], [], first
    for (h, w), al in zip(sizes, align):
        if al == 16:
            at = -(-at // 16) * 16
        elif al == 1:
            at |= 1
        n = h * w * 3
        views.append(arena[at:at + n].view(h, w, 3))
        spans.append((at, n))
        at += n + guard
    assert at <= arena.numel()
    return views, spans


def guards_untouched(arena, spans, poison):
    keep = torch.ones(arena.numel(), dtype=torch.bool)
    for at, n in spans:
        keep[at:at + n] = False
    return bool((arena.cpu()[keep] == poison).all())


def raw_call(hip, B, src, dst, h, w, s_gain, v_gain):
    """The entry point's return code, with nothing between the caller and the argument block."""
    n = hip.BATCH_STAGE_MAX_B
    a = hip.HsvJitterArgs(B=B, src=(ctypes.c_void_p * n)(*src), dst=(ctypes.c_void_p * n)(*dst), h=(ctypes.c_int32 * n)(*h),
                          w=(ctypes.c_int32 * n)(*w), s_gain=(ctypes.c_float * n)(*s_gain), v_gain=(ctypes.c_float * n)(*v_gain))
    return hip.lib().rt_hsv_jitter(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("gains", [(1.0, 1.0), (1.0, 0.5), (1.0, 1.4999), (0.62, 1.27)])
def test_all_colours_equal_the_definition(hip, all_colours, gains):
    img, dev = all_colours
    out = torch.empty_like(dev)
    hip.hsv_jitter([dev], [gains], [out])
    want = jitter.apply(img, *gains)
    got = out.cpu()
    n = int((got != want).sum())
    print(f"\n[hsv jitter] gains {gains}: {n} of {got.numel()} bytes differ from jitter.apply")
    assert n == 0
    assert torch.equal(dev.cpu(), img)                                    # the source is only read


def test_addressing_guards_in_place_and_a_second_batch(hip):
    poison = 0xA5
    arena = torch.full((32768,), poison, dtype=torch.uint8, device="cuda")
    src_arena = torch.zeros(32768, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0 and src_arena.data_ptr() % 16 == 0
    for sizes, gains, dst_align, src_align, seed in ((SIZES_A, GAINS_A, (None, 1, 16, None, 16), (16, None, 16, 1, 16), 1),
                                                    (SIZES_B, GAINS_B, (16, 16, None, 1, None), (None, 16, 1, 16, None), 2)):
        host = host_images(sizes, seed)
        want = [jitter.apply(im, *g) for im, g in zip(host, gains)]
        srcs, _ = carve(src_arena, sizes, src_align)
        for s, im in zip(srcs, host):
            s.copy_(im)
        arena.fill_(poison)
        dsts, spans = carve(arena, sizes, dst_align)
        assert any(d.data_ptr() % 2 for d in dsts) and any(s.data_ptr() % 2 for s in srcs)                  # an odd base on either side
        assert any(d.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0 for d, s in zip(dsts, srcs))         # and a pair of aligned ones
        hip.hsv_jitter(srcs, gains, dsts)
        torch.cuda.synchronize()
        for k, (d, s, w, im) in enumerate(zip(dsts, srcs, want, host)):
            assert torch.equal(d.cpu(), w), (sizes[k], "output")
            assert torch.equal(s.cpu(), im), (sizes[k], "source")
        assert guards_untouched(arena, spans, poison)
        # in place: dst[b] == src[b]
        keep = src_arena.clone()
        hip.hsv_jitter(srcs, gains, srcs)
        torch.cuda.synchronize()
        for k, (s, w) in enumerate(zip(srcs, want)):
            assert torch.equal(s.cpu(), w), (sizes[k], "in place")
        touched = torch.zeros(src_arena.numel(), dtype=torch.bool)
        for s in srcs:
            at = s.data_ptr() - src_arena.data_ptr()
            touched[at:at + s.numel()] = True
        assert torch.equal(src_arena.cpu()[~touched], keep.cpu()[~touched])


def test_batch_limits(hip):
    n = hip.BATCH_STAGE_MAX_B
    assert n == 64
    host = host_images([(2, 3)] * n, 3)
    gains = [(1.0, 0.5 + b / 64.0) for b in range(n)]
    dev = [im.cuda() for im in host]
    outs = [torch.empty_like(d) for d in dev]
    hip.hsv_jitter(dev, gains, outs)
    torch.cuda.synchronize()
    for b in range(n):
        assert torch.equal(outs[b].cpu(), jitter.apply(host[b], *gains[b])), b
    before = [o.clone() for o in outs]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    assert raw_call(hip, n + 1, ptr(dev), ptr(outs), [2] * n, [3] * n, [1.0] * n, [1.0] * n) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, before))


def test_bad_arguments_launch_nothing(hip):
    src = torch.randint(0, 256, (2, 7, 9, 3), dtype=torch.uint8).cuda()
    dst = torch.full((2, 7, 9, 3), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(B=2, src=[src[0].data_ptr(), src[1].data_ptr()], dst=[dst[0].data_ptr(), dst[1].data_ptr()], h=[7, 7], w=[9, 9],
                s_gain=[1.0, 1.0], v_gain=[0.8, 1.2])
    for kw in (dict(v_gain=[0.8, -0.1]), dict(s_gain=[-0.1, 1.0]), dict(v_gain=[float("nan"), 1.2]), dict(s_gain=[1.0, float("nan")]),
               dict(v_gain=[0.8, float("inf")]), dict(s_gain=[float("inf"), 1.0]), dict(src=[src[0].data_ptr(), None]),
               dict(dst=[None, dst[1].data_ptr()]), dict(h=[7, 0]), dict(w=[0, 9]), dict(h=[-7, 7]), dict(B=0)):
        assert raw_call(hip, **dict(good, **kw)) == BAD, kw
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    assert raw_call(hip, **good) == 0                                     # ... and the block they were made from is a good one
    torch.cuda.synchronize()
    assert torch.equal(dst[1].cpu(), jitter.apply(src[1].cpu(), 1.0, 1.2)) and torch.equal(dst[0].cpu(), jitter.apply(src[0].cpu(), 1.0, 0.8))


def test_the_same_bits_from_run_to_run(hip):
    host = host_images([(97, 131), (200, 300), (3, 5)], 4)
    gains = [(1.0, 0.77), (0.62, 1.27), (1.0, 1.1)]
    dev = [im.cuda() for im in host]
    a, b = [torch.empty_like(d) for d in dev], [torch.empty_like(d) for d in dev]
    hip.hsv_jitter(dev, gains, a)
    hip.hsv_jitter(dev, gains, b)
    torch.cuda.synchronize()
    for x, y, im, g in zip(a, b, host, gains):
        assert torch.equal(x, y) and torch.equal(x.cpu(), jitter.apply(im, *g))
