"""GPU: DeviceInputPipeline(pad_to=(H, W)) collates straight to a canvas size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_pad_to_is_the_own_size_batch_padded(hip):
    from reftr_amd.data import DeviceInputPipeline
    rng = np.random.default_rng(11)
    imgs = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for h, w in [(120, 160), (97, 211)]]
    own, _ = DeviceInputPipeline(size=64, max_size=64)(imgs)
    h, w = own.tensors.shape[-2:]
    assert (h, w) != (64, 80)
    nt, _ = DeviceInputPipeline(size=64, max_size=64, pad_to=(64, 80))(imgs)
    assert tuple(nt.tensors.shape) == (2, 3, 64, 80) and tuple(nt.mask.shape) == (2, 64, 80) and nt.mask.dtype == torch.bool
    assert torch.equal(nt.tensors[:, :, :h, :w], own.tensors) and torch.equal(nt.mask[:, :h, :w], own.mask)
    assert not nt.tensors[:, :, h:, :].any() and not nt.tensors[:, :, :, w:].any()
    assert nt.mask[:, h:, :].all() and nt.mask[:, :, w:].all()
    with pytest.raises(ValueError, match="pad_to"):
        DeviceInputPipeline(size=64, max_size=64, pad_to=(h - 1, 80))(imgs)
