"""Raw batches: the decoded uint8 images of a batch as they are, with the `size` / `max_size` they are to be resized to.

A loader that delivers `samples["img"]` as a RawImages -- and targets in the RAW frame: `boxes` xyxy in pixels, for RES a one-byte
[1, h, w] `masks` -- leaves resize, ToTensor, Normalize, the collate's padding and the target transforms of datasets/transforms.py to the
device: engine_vg's steps take such a batch whenever `canvas=` is given, and BatchCanvas.stage writes it into the captured step's buffers
with one rt_raw_stage launch.  The only image bytes that cross to the device are the raw ones.  What a raw batch MEANS is
BatchCanvas.pad_on_host: the DeviceInputPipeline chain, then the canvas's padding.

The one stochastic transform of the reference's training recipe, RandomIntensitySaturation, travels with the batch as per-image gains
(`RawImages.gains`, `raw_collate(jitter=True)`): reftr_amd.data.jitter defines what they do to the bytes, and the device does it to the
raw images in front of the resize (rt_hsv_jitter).  A batch without gains is the batch it always was."""
import math

import torch

from . import resample
from .jitter import draw_gains


class RawImages:
    """B uint8 [h, w, 3] images of any sizes, and the resize they ask for (RandomResize([size], max_size))."""

    def __init__(self, images, size, max_size=None, gains=None):
        """`gains`: None, or B (s_gain, v_gain) host floats -- the colour jitter (reftr_amd.data.jitter) the device applies to the raw
        bytes in front of the resize (rt_hsv_jitter); a training augmentation, refused by evaluation and prediction."""
        self.images, self.size, self.max_size = list(images), int(size), None if max_size is None else int(max_size)
        self.gains = None if gains is None else [(float(s), float(v)) for s, v in gains]
        self._out = None

    def __len__(self):
        return len(self.images)

    @property
    def device(self):
        return self.images[0].device

    @property
    def is_cuda(self):
        return all(im.is_cuda for im in self.images)

    def well_formed(self):
        if self.gains is not None and (len(self.gains) != len(self.images)
                                       or not all(math.isfinite(g) and g >= 0.0 for pair in self.gains for g in pair)):
            return False
        return bool(self.images) and all(torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
                                         and im.shape[0] > 0 and im.shape[1] > 0 for im in self.images)

    def out_sizes(self):
        """[(oh, ow)] of the resized images: resample.size_with_aspect_ratio, the one definition (host integers, computed once)."""
        if self._out is None:
            self._out = [resample.size_with_aspect_ratio(int(im.shape[1]), int(im.shape[0]), self.size, self.max_size) for im in self.images]
        return self._out

    def to(self, device, non_blocking=False):
        out = RawImages([im.to(device, non_blocking=non_blocking) for im in self.images], self.size, self.max_size, self.gains)
        out._out = self._out
        return out

    def pin_memory(self):
        """(what a DataLoader with pin_memory=True calls on a batch field it does not know)"""
        out = RawImages([im.pin_memory() for im in self.images], self.size, self.max_size, self.gains)
        out._out = self._out
        return out

    def record_stream(self, stream):
        for im in self.images:
            if im.is_cuda:
                im.record_stream(stream)


def raw_collate(size, max_size=None, jitter=False):
    """A DataLoader collate_fn for items (image uint8 [h, w, 3], token fields {name: tensor}, target {boxes xyxy pixels, masks ...}):
    -> (samples, targets) with samples["img"] a RawImages and the token fields stacked; images and targets are not touched.
    `jitter`: the batch carries the reference's RandomIntensitySaturation as per-image gains (jitter.draw_gains, two random() draws per
    image in the reference's order); the device applies them."""
    def collate(items):
        images, fields, targets = zip(*items)
        samples = {k: torch.stack([f[k] for f in fields]) for k in fields[0]}
        samples["img"] = RawImages([torch.as_tensor(im) for im in images], size, max_size,
                                   gains=draw_gains(len(images)) if jitter else None)
        return samples, [dict(t) for t in targets]
    return collate
