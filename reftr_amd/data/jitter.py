"""The reference's colour jitter, RandomIntensitySaturation (datasets/transforms.py:266-285), as a definition in plain torch on the
CPU: per image an 8-bit RGB -> HSV conversion, a gain on V (and, through the ABI, on S), and the 8-bit conversion back.  The
reference does this with cv2; this module restates OpenCV's scalar 8-bit paths operation for operation -- integers with hsv_shift =
12 on the way in, fp32 without any fused multiply-add on the way out -- and the device kernel rt_hsv_jitter is held to it bit for bit
(tests/test_jitter_gpu.py).  It has NOT been pinned against a cv2 build: none is available where this package is built and tested, and
OpenCV builds differ among themselves in whether the fp32 products are contracted.  The jitter is a stochastic augmentation; what is
fixed here is that the kernel equals this text.

What the reference's transform does: it draws a1 and a2 = (random.random() * 2 - 1) * 0.5 + 1; a1 only ever CLIPS S (when a1 > 1) and
never multiplies it, so S is unchanged; V = float32(V) * a2, clipped to [0, 255] only when a2 > 1, then truncated to uint8.
`draw_gains` therefore returns (1.0, a2).  The round trip alone moves bytes: gains (1, 1) are not the identity.

No device and no kernel library is used here."""
import functools
import random

import torch

HSV_SHIFT = 12
# (b, g, r) = tab[SECTORS[sector]] (OpenCV's sector_data)
SECTORS = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))


@functools.lru_cache(maxsize=None)
def tables():
    """(sdiv, hdiv) int32 [256]: rint((255 << 12) / (1.0 * i)) and rint((180 << 12) / (6.0 * i)) -- a double division, rounded half to
    even -- and 0 at i = 0."""
    i = torch.arange(1, 256, dtype=torch.float64)
    sdiv, hdiv = torch.zeros(256, dtype=torch.int32), torch.zeros(256, dtype=torch.int32)
    sdiv[1:] = torch.round(float(255 << HSV_SHIFT) / (1.0 * i)).to(torch.int32)
    hdiv[1:] = torch.round(float(180 << HSV_SHIFT) / (6.0 * i)).to(torch.int32)
    return sdiv, hdiv


def rgb_to_hsv(img):
    """uint8 [..., 3] RGB -> (h, s, v) int32 [...]: H in [0, 180), S and V in [0, 255]."""
    sdiv, hdiv = tables()
    r, g, b = img.to(torch.int32).unbind(-1)
    v = torch.maximum(r, torch.maximum(g, b))
    d = v - torch.minimum(r, torch.minimum(g, b))
    half = 1 << (HSV_SHIFT - 1)
    s = (d * sdiv[v.long()] + half) >> HSV_SHIFT
    h0 = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * hdiv[d.long()] + half) >> HSV_SHIFT          # an arithmetic shift: h0 may be negative
    return torch.where(h < 0, h + 180, h), s, v


def _gain(x, gain):
    """int32 in [0, 255] -> int32 in [0, 255]: (uint8)(int)((float)x * gain), clipped to [0, 255] only when gain > 1; `gain` is taken
    as the fp32 the ABI carries."""
    g = torch.tensor(float(gain), dtype=torch.float32)
    assert bool(torch.isfinite(g)) and float(g) >= 0.0, gain
    if float(g) == 1.0:
        return x                                           # (the product is exact: the byte as it is)
    y = x.to(torch.float32) * g
    if float(g) > 1.0:
        y = y.clamp(0.0, 255.0)
    return y.to(torch.int32)                               # truncation; [0, 255] already


def hsv_to_rgb(h, s, v):
    """(h, s, v) integer tensors [...] -> uint8 [..., 3] RGB.  Every product and every difference is its own fp32 operation."""
    f32 = torch.float32
    h_scale = torch.tensor(6.0, dtype=f32) / torch.tensor(180.0, dtype=f32)
    inv255 = torch.tensor(1.0, dtype=f32) / torch.tensor(255.0, dtype=f32)
    hf, sf, vf = h.to(f32) * h_scale, s.to(f32) * inv255, v.to(f32) * inv255
    fl = torch.floor(hf)
    sector, f = fl.to(torch.int32), hf - fl
    outside = (sector < 0) | (sector > 5)
    sector, f = sector.masked_fill(outside, 0), f.masked_fill(outside, 0.0)
    tab = (vf, vf * (1.0 - sf), vf * (1.0 - sf * f), vf * (1.0 - sf * (1.0 - f)))
    grey = s == 0
    out = []
    for ch in (2, 1, 0):                                   # r, g, b of the (b, g, r) rows
        c = tab[SECTORS[5][ch]]
        for k in range(4, -1, -1):
            c = torch.where(sector == k, tab[SECTORS[k][ch]], c)
        c = torch.where(grey, vf, c)
        out.append(torch.round(c * 255.0).clamp(0.0, 255.0).to(torch.uint8))          # rintf: round half to even
    return torch.stack(out, dim=-1)


def apply(img, s_gain, v_gain):
    """uint8 [h, w, 3] -> uint8 [h, w, 3]: the round trip with S scaled by s_gain and V by v_gain (host floats, taken as fp32)."""
    assert img.dtype == torch.uint8 and img.shape[-1] == 3
    h, s, v = rgb_to_hsv(img)
    return hsv_to_rgb(h, _gain(s, s_gain), _gain(v, v_gain))


def draw_gains(n, rng=random):
    """The gains of n images as the reference draws them: per image two random() calls, a1 then a2.  a1 is consumed and, as in the
    reference, has no effect: [(1.0, a2)] * n."""
    out = []
    for _ in range(n):
        rng.random()                                       # a1: drawn, then only ever clips S
        out.append((1.0, (rng.random() * 2 - 1) * 0.5 + 1))
    return out
