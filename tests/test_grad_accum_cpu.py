"""CPU: the bookkeeping of gradient accumulation in reftr_amd.optim (window counter, s = 1 / r, lazy accumulator, refusals) on a
CPU store.  No kernel runs: hip.grad_accum is replaced by a recorder."""
import types

import pytest
import torch


def small_model():
    from reftr_amd.models import layout as L
    from reftr_amd.models.reftr_transformer import RefTR
    cfg = L.ModelConfig(enc_layers=1, dec_layers=1, bert=L.BertConfig(layers=1), resnet_layers=(1, 1, 1, 1))
    return RefTR(cfg, device="cpu")


@pytest.fixture()
def recorded(monkeypatch):
    from reftr_amd import hip
    calls = []

    def grad_accum(mode, g, acc, scale=1.0, scale_dev=None, partials=None, out_sq=None):
        calls.append(types.SimpleNamespace(mode=mode, g=g, acc=acc, scale=scale, partials=partials, out_sq=out_sq))
    monkeypatch.setattr(hip, "grad_accum", grad_accum)
    return calls


@pytest.mark.parametrize("sgd", [False, True])
def test_window_counter_scale_and_lazy_accumulator(recorded, sgd):
    from reftr_amd import hip
    from reftr_amd.optim import FusedAdamW, FusedSGD
    m = small_model()
    opt = (FusedSGD if sgd else FusedAdamW)(m)
    st = m.store
    assert opt.accum is None and opt.accum_count == 0
    # a window of one micro-batch: nothing accumulated, nothing launched, nothing allocated -- the plain step follows
    assert opt.finish_accumulation() == 1.0
    assert recorded == [] and opt.accum is None and not opt._window_sq
    for r in (2, 3, 5):
        del recorded[:]
        st.norm_valid = True
        for i in range(r - 1):
            assert opt.accumulate() == i + 1
            assert not st.norm_valid and m._norm_split is None     # the epilogue-collected norm is one micro-batch's: dropped
        assert opt.accum_count == r - 1
        acc = opt.accum
        assert acc is not None and acc.shape == st.flat_g.shape and acc.dtype == torch.float32 and acc.device == st.flat_g.device
        st.norm_valid = True
        s = opt.finish_accumulation()
        assert s == 1.0 / r and opt.accum_count == 0 and not st.norm_valid
        assert [c.mode for c in recorded] == [hip.ACCUM_FIRST] + [hip.ACCUM_ADD] * (r - 2) + [hip.ACCUM_FINISH]
        assert all(c.g is st.flat_g and c.acc is acc for c in recorded)            # one accumulator, allocated once
        fin = recorded[-1]
        assert fin.scale == 1.0 / r and fin.out_sq is opt.sq and fin.partials.numel() >= hip.GRAD_ACCUM_SLOTS
        # self.sq is the window's squared norm: the clip that follows takes it as it is, once
        assert opt._window_sq
        opt._sqnorm_all()
        assert not opt._window_sq and len(recorded) == r
    assert opt.step_count == 0                        # accumulating never advances the step counter
    # a finished window that no clip / step consumed does not outlive the next backward's gradient clear (a capture started in that
    # state would otherwise leave its norm launch out of the graph)
    opt.accumulate(); opt.finish_accumulation()
    assert opt._window_sq
    opt.zero_grad(fast=True)
    assert not opt._window_sq


def test_state_dict_inside_a_window_is_refused(recorded):
    from reftr_amd.optim import FusedAdamW, FusedSGD
    for cls in (FusedAdamW, FusedSGD):
        opt = cls(small_model())
        opt.state_dict()
        opt.accumulate()
        with pytest.raises(RuntimeError, match="accumulation window"):
            opt.state_dict()
        opt.finish_accumulation()
        opt.state_dict()


def test_data_parallel_and_bf16_exchange_are_refused(recorded):
    from reftr_amd.engine_vg import train_step
    from reftr_amd.optim import FusedAdamW
    m = small_model()
    opt = FusedAdamW(m)
    m.store.flat_g16 = torch.zeros(4, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bf16 gradient"):
        opt.accumulate()
    m.store.flat_g16 = None
    m._stops = frozenset(["main"])                    # what an active data-parallel wrapper's capture sets: dp_mode
    assert m.dp_mode
    with pytest.raises(NotImplementedError, match="data-parallel"):
        train_step(m, None, None, None, opt, accum_steps=2)          # refused before anything runs
    m._stops = frozenset()
    with pytest.raises(NotImplementedError, match="FusedAdamW"):
        train_step(m, None, None, None, torch.optim.SGD(m.parameters(), lr=0.1), accum_steps=2)
    assert recorded == [] and opt.accum is None


def test_build_optimizer_takes_the_flag():
    from reftr_amd.optim import build_optimizer
    m = small_model()
    args = types.SimpleNamespace(lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    assert build_optimizer(m, args).accum_steps == 1
    args.accum_steps = 8
    assert build_optimizer(m, args).accum_steps == 8
    args.accum_steps = 0
    with pytest.raises(ValueError):
        build_optimizer(m, args)
