"""Train / eval loops with the reference's signatures (engine_vg.py:22-25,82): the loop body of
train_one_epoch is the hot path this library accelerates (engine_vg.py:40-72).

Differences that are deliberate and documented in INTEGRATION.md:
  * `optimizer` is reftr_amd.optim.FusedAdamW (clip + AdamW in one kernel); a plain torch optimizer also works;
  * the prefetcher only uses a side HIP stream when the device is a GPU (the reference constructs
    torch.cuda.Stream() unconditionally, engine_vg.py:240).
"""
import math
import contextlib
import os
import sys

import torch

from . import hip as H
from .data.raw import RawImages
from .metrics import EvalMeter, decode_ring
from .util import misc as utils
from .util.box_ops import box_cxcywh_to_xyxy, box_iou, mask_iou


def _to_device(samples, targets, device, non_blocking=True):
    s = {k: (v.to(device, non_blocking=non_blocking) if hasattr(v, "to") else v) for k, v in samples.items()}
    t = [{k: (v.to(device, non_blocking=non_blocking) if hasattr(v, "to") else v) for k, v in tg.items()} for tg in targets]
    return s, t


class data_prefetcher:
    """H2D copies on a side stream, one batch ahead (engine_vg.py:234-291)."""

    def __init__(self, loader, device, prefetch=True):
        self.loader = iter(loader)
        self.device = torch.device(device)
        self.prefetch = prefetch and self.device.type == "cuda"
        if self.prefetch:
            self.stream = torch.cuda.Stream()
            self.preload()

    def preload(self):
        try:
            s, t = next(self.loader)
        except StopIteration:
            self.next_samples = self.next_targets = None
            return
        with torch.cuda.stream(self.stream):
            self.next_samples, self.next_targets = _to_device(s, t, self.device)

    def next(self):
        if not self.prefetch:
            try:
                s, t = next(self.loader)
            except StopIteration:
                return None, None
            return _to_device(s, t, self.device, non_blocking=False)
        torch.cuda.current_stream().wait_stream(self.stream)
        s, t = self.next_samples, self.next_targets
        if s is not None:
            for v in s.values():
                if hasattr(v, "record_stream"):
                    v.record_stream(torch.cuda.current_stream())
            for tg in t:
                for v in tg.values():
                    if hasattr(v, "record_stream"):
                        v.record_stream(torch.cuda.current_stream())
        self.preload()
        return s, t


def _total(criterion, loss_dict):
    """engine_vg.py:43.  The HIP criterion offers the same weighted sum as one fused reduction."""
    if hasattr(criterion, "weighted_total") and os.environ.get("REFTR_FUSED_TOTAL", "1") != "0":
        return criterion.weighted_total(loss_dict)
    wd = criterion.weight_dict
    return sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)


def _zero_grad(optimizer):
    """engine_vg.py:60.  The fused optimizer clears only what backward accumulates with atomics (the weight matrices are
    overwritten by their producers); any other optimizer: the plain zero_grad()."""
    if isinstance(getattr(optimizer, "model", None), torch.nn.Module) and hasattr(optimizer, "apply_pending"):
        optimizer.zero_grad(fast=True)
    else:
        optimizer.zero_grad()


def _inner(model):
    return getattr(model, "module", model)


def _multi_rank():
    return utils.is_dist_avail_and_initialized() and utils.get_world_size() > 1


class _StepState:
    """What the step machinery keeps per model beside `model._captured_steps`: the capture that holds the staged next batch, the
    count of cooperative-decoder fall-backs (CapturedForward drops its graphs when it moves), and what was already said once."""

    def __init__(self):
        self.staged_cap, self.coop_generation, self.said = None, 0, set()


def _state(model):
    d = _inner(model).__dict__
    st = d.get("_step_state")
    if st is None:
        st = d["_step_state"] = _StepState()
    return st


def _say_once(model, key, text):
    said = _state(model).said
    if key not in said:
        said.add(key)
        print(text, file=sys.stderr)


def _seed_state(model):
    """(device dropout step-seed word, host step count) BEFORE this iteration's forward advanced them (train_step reads them
    after the forward: one step back)."""
    inner = _inner(model)
    if not hasattr(inner, "seed_dev"):
        return None
    return (1 if inner.training else 0, 1)


def _restore_seed(model, back):
    """Takes back the dropout-seed / step advance of an iteration that is run again."""
    inner = _inner(model)
    if back is None:
        return
    if back[0]:
        inner.seed_dev.sub_(back[0])
    inner._step -= back[1]


def _cooperative_failed(model):
    """True when a cooperative decoder launch of THIS process -- or, under data parallelism, of any rank (the choice to run the
    iteration again must be collective) -- raised its failure word since it was last cleared.  One host read (eager loop only; the
    replayed loop carries the word in its per-iteration stats vector)."""
    inner = _inner(model)
    fw = inner.coop_failure_word() if hasattr(inner, "coop_failure_word") else None
    if fw is None:                                     # no cooperative launches in this build / configuration: the same on every rank
        return False
    launched = getattr(inner.net, "dec_counters", None) is not None      # rank-local (depends on this rank's batch shape)
    if _multi_rank():
        # every rank enters the collective; a rank that has not launched the cooperative decoder yet contributes 0
        f = fw.to(torch.int32).clone() if launched else torch.zeros_like(fw, dtype=torch.int32)
        torch.distributed.all_reduce(f, op=torch.distributed.ReduceOp.MAX)
        return int(f) != 0
    return launched and int(fw) != 0


_COOP_LOGGED = False


def _coop_fallback(model):
    """Switches the cooperative decoder launches off for this process (the launched chain computes the same values), clears the
    failure word, and drops every captured step / forward of the model: they contain the launches.  Pending (deferred) updates of
    the dropped captures are discarded -- the caller runs the failed iteration again."""
    global _COOP_LOGGED
    inner = _inner(model)
    net = inner.net
    net.dec_coop = net.dec_coop_bwd = False
    os.environ["REFTR_DEC_COOP"] = "0"; os.environ["REFTR_DEC_COOP_BWD"] = "0"
    if net._dec_handoff is not None:
        net._dec_handoff[1:2].zero_()
    net.dec_counters = None
    caps = inner.__dict__.get("_captured_steps") or {}
    for cap in caps.values():
        cap.reset_pending()
        if getattr(cap.optimizer, "veto", None) is not None:
            cap.optimizer.veto = None
    caps.clear()
    state = _state(model)
    state.staged_cap = None
    state.coop_generation += 1                         # CapturedForward drops its graphs
    if not _COOP_LOGGED:
        _COOP_LOGGED = True
        print("[reftr_amd] rt_decoder_fwd / rt_decoder_bwd: a stage hand-off timed out (workgroups not co-resident?). The iteration "
              "is discarded and run again; the decoder uses the launched chain (REFTR_DEC_COOP=0) from here on.", file=sys.stderr)


def _run_again_on_chain(model, run, drop=None):
    """run(); when a cooperative decoder hand-off timed out in it, what it produced is void: the launches are switched off
    (_coop_fallback), the caller drops what it must (`drop`: captures that contain the launches, an advanced dropout seed) and run()
    is called once more, on the launched chain -- at most once, its result is not asked again.  Returns the result that stands."""
    out = run()
    if _cooperative_failed(model):
        _coop_fallback(model)
        if drop is not None:
            drop()
        out = run()
    return out


def _require_accumulation(optimizer):
    """accum_steps > 1 needs the fused optimizer's accumulator, on a single-process fp32 gradient buffer."""
    if not hasattr(optimizer, "finish_accumulation"):
        raise NotImplementedError("accum_steps > 1 needs reftr_amd.optim.FusedAdamW / FusedSGD (the gradient buffer is assigned, not "
                                  "added to, by each backward: a foreign optimizer cannot accumulate it)")
    optimizer.check_accumulation()


def _window_last(optimizer, accum_steps, window_end):
    """Whether the micro-batch about to run closes its accumulation window: the caller says so (`window_end`, e.g. the last batch
    of an epoch), or it is the accum_steps-th one since the last update."""
    if window_end is not None:
        return bool(window_end)
    return optimizer.accum_count + 1 >= accum_steps


def _canvas_single_process(model):
    inner = _inner(model)
    if model is not inner or getattr(inner, "dp_mode", False) or _multi_rank():
        raise NotImplementedError("canvas= is not available under the data-parallel wrapper: the box count a canvas step reads is the "
                                  "world average (one all-reduce per batch) and the choice between replay and capture is collective; "
                                  "neither has been run on more than one rank with a canvas")


def _canvas_fits(model, canvas, samples, targets):
    """Whether this batch goes through the batch canvas (reftr_amd.data.canvas).  A batch that does not fit -- a larger image, more
    boxes than the capacity, other token lengths -- takes the existing path at its own shape; said once per shape, because a run
    that quietly leaves the canvas pays a capture or the eager launches (2-3x slower) for every such batch."""
    _canvas_single_process(model)
    why = canvas.why_not(samples, targets)
    if why is None:
        return True
    key = CapturedTrainStep.shape_key(samples, targets) if isinstance(samples.get("img"), utils.NestedTensor) else why
    _say_once(model, ("canvas", key), f"[reftr_amd] batch does not fit {canvas!r} ({why}): it runs at its own shape, captured if fewer "
              "than max_shapes shapes are in use, else eagerly")
    return False


def _is_raw(samples):
    return isinstance(samples, dict) and isinstance(samples.get("img"), RawImages)


def _no_gains(samples, batch_no):
    """evaluate_raw's refusal of a raw batch that carries the colour jitter (RawImages.gains), before anything of it is launched."""
    if samples["img"].gains is not None:
        raise ValueError(f"evaluate_raw: batch {batch_no} carries gains (RawImages.gains): the colour jitter is a training augmentation, "
                         "and an evaluation that applied it would silently score other images")


def _on_device(samples):
    """Whether the batch's image -- a NestedTensor, or a raw batch's RawImages -- is in device memory."""
    img = samples.get("img")
    return img.is_cuda if isinstance(img, RawImages) else isinstance(img, utils.NestedTensor) and img.tensors.is_cuda


def _raw_batch(model, canvas, samples, targets):
    """A raw batch (reftr_amd.data.raw) at the door of a step: -> (samples, targets, canvas) as the step machinery takes them.  One
    that fits the canvas goes on as it is: BatchCanvas.stage writes it with one rt_raw_stage launch.  One that does not is converted
    once by the existing device chain (BatchCanvas.resized) and takes the existing path at its own shape, without the canvas; said
    once per reason.  Without a canvas there is nowhere to stage it: refused."""
    if not _is_raw(samples):
        return samples, targets, canvas
    if canvas is None:
        raise NotImplementedError("a raw batch (reftr_amd.data.RawImages) needs canvas=: rt_raw_stage writes it into a canvas's "
                                  "buffers; without one, run reftr_amd.data.DeviceInputPipeline in the loader's collate")
    _canvas_single_process(model)
    cap = _state(model).staged_cap
    if cap is not None and cap._staged is not None and cap._staged[0] is samples:
        return samples, targets, canvas               # checked when the previous iteration's lookahead staged it
    if not samples["img"].is_cuda:                    # a host batch: the raw bytes cross, everything else happens on the device
        samples, targets = _to_device(samples, targets, _inner(model).store.device)
    why = canvas.why_not(samples, targets)
    if why is None:
        return samples, targets, canvas
    _say_once(model, ("canvas", why), f"[reftr_amd] raw batch does not fit {canvas!r} ({why}): it is resized by the DeviceInputPipeline "
              "chain and runs at its own shape, captured if fewer than max_shapes shapes are in use, else eagerly")
    return (*canvas.resized(samples, targets), None)


_UNSCALED = "{}_unscaled".format          # a loss term's name on the stats board beside its weighted value


def _read_out(values, weight_dict):
    """The loop's read-out of one iteration (engine_vg.py:46-58): named loss values -- reduced device scalars on the eager path, host
    floats on the replayed one -- to (loss_value, weighted dict, unweighted dict); a non-finite total stops the run before the update.
    loss_value is a Python float either way (one .item() for device scalars); the dicts keep the type of what came in."""
    unscaled = {_UNSCALED(k): v for k, v in values.items()}
    scaled = {k: v * weight_dict[k] for k, v in values.items() if k in weight_dict}
    loss_value = sum(scaled.values())
    on_device = torch.is_tensor(loss_value)
    if on_device:
        loss_value = loss_value.item()
    if not math.isfinite(loss_value):
        print("Loss is {}, stopping training".format(loss_value))
        print(values if on_device else unscaled)
        sys.exit(1)
    return loss_value, scaled, unscaled


def _eager_iteration(model, criterion, samples, targets, optimizer):
    """Forward, criterion, total, the reduced read-out with its non-finite stop, gradient clear and backward of one (micro-)batch:
    what train_step runs once, and once more after a cooperative decoder fall-back.  Returns what _read_out returns."""
    outputs = model(samples)
    loss_dict = criterion(outputs, targets)
    losses = _total(criterion, loss_dict)
    res = _read_out(utils.reduce_dict(loss_dict), criterion.weight_dict)
    _zero_grad(optimizer)
    losses.backward()
    return res


def _train_step_canvas(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, accum_steps, window_end, canvas):
    """train_step on the canvas form of the batch: staged by rt_batch_stage into fresh buffers (device batches; the criterion reads
    the staged targets), or padded by canvas.pad_on_host (host batches).  The same step as `train_step` of the padded batch."""
    if not (_on_device(samples) and hasattr(criterion, "targets_static")):
        samples, targets = canvas.pad_on_host(samples, targets)
        return train_step(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, accum_steps, window_end)
    staged = canvas.stage(samples, targets)
    criterion.targets_static, criterion.target_masks_static = staged.targets_static, staged.tgt_masks
    try:
        return train_step(model, criterion, staged.samples, targets, optimizer, lr_scheduler, max_norm, accum_steps, window_end)
    finally:
        criterion.targets_static = criterion.target_masks_static = None


def train_step(model, criterion, samples, targets, optimizer, lr_scheduler=None, max_norm=0.0, accum_steps=1, window_end=None,
               canvas=None):
    """The loop body, engine_vg.py:40-72.  Returns (loss_value, reduced scaled dict, reduced unscaled dict,
    grad_norm tensor).

    canvas (a reftr_amd.data.canvas.BatchCanvas): the step is computed on the batch padded to the canvas -- what a replayed canvas
    step computes; a batch that does not fit the canvas runs as without one.

    accum_steps = k > 1 (gradient accumulation: the published 8 x 8 global batch on one GPU): the call is ONE micro-batch of a
    window of k.  Micro-batches 1 ... k-1 run forward, criterion, the fast zero_grad, backward and optimizer.accumulate(); they
    neither clip, update nor step the scheduler, and return None as their gradient norm.  The k-th (or any call with
    window_end=True: a window cut short by the end of the epoch holds r < k micro-batches) averages the window's gradients
    (optimizer.finish_accumulation(), s = 1 / r), then clips, updates and steps the scheduler ONCE and returns the norm of the
    averaged gradient.  The non-finite-loss stop and the cooperative decoder's re-run act on every micro-batch."""
    accum_steps = int(accum_steps)
    samples, targets, canvas = _raw_batch(model, canvas, samples, targets)
    if canvas is not None and _canvas_fits(model, canvas, samples, targets):
        return _train_step_canvas(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, accum_steps, window_end, canvas)
    if accum_steps > 1:
        _require_accumulation(optimizer)
    if hasattr(optimizer, "veto") and hasattr(_inner(model), "coop_failure_word"):
        optimizer.veto = _inner(model).coop_failure_word()
    # a stage hand-off of the cooperative decoder launches that timed out voids this iteration's activations / gradients.  The
    # reference stops BEFORE the update when an iteration is bad (engine_vg.py:55-58); here the launches are switched off for the
    # process and the iteration is run again on the launched chain (same dropout seeds), then updated as usual
    res = _run_again_on_chain(model, lambda: _eager_iteration(model, criterion, samples, targets, optimizer),
                              drop=lambda: _restore_seed(model, _seed_state(model)))
    last = _window_last(optimizer, accum_steps, window_end) if accum_steps > 1 else None
    return (*res, _update(model, optimizer, lr_scheduler, max_norm, last))


def _update(model, optimizer, lr_scheduler, max_norm, last=None, sync_lr=False):
    """What follows an iteration's backward, eager or replayed; returns the gradient norm.  `last` says that the iteration is a
    micro-batch of an accumulation window and whether it closes it: inside the window the gradients go to the accumulator and
    nothing else happens (None); the last one averages the window first.  Then clip, update and scheduler step, once."""
    if last is not None:
        if not last:
            optimizer.accumulate()
            return None
        optimizer.finish_accumulation()
    if sync_lr and getattr(optimizer, "lr_dev", None) is not None:
        optimizer.sync_lr()                  # a capture of this optimizer switched the kernel to device learning rates
    if hasattr(optimizer, "clip_grad_norm_"):
        grad_total_norm = optimizer.clip_grad_norm_(max_norm)
    elif max_norm > 0:
        grad_total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    else:
        grad_total_norm = torch.zeros(())
    optimizer.step()
    if lr_scheduler is not None:
        lr_scheduler.step()
    return grad_total_norm


def _sample_shapes(samples):
    """((field, shape), ...) of a batch's samples: what a capture's static input buffers are sized by."""
    return tuple((n, tuple(v.tensors.shape) if isinstance(v, utils.NestedTensor) else tuple(v.shape))
                 for n, v in sorted(samples.items()) if isinstance(v, utils.NestedTensor) or torch.is_tensor(v))


def _clone_batch(samples, targets):
    def c(v):
        if isinstance(v, utils.NestedTensor):
            return utils.NestedTensor(v.tensors.clone(), v.mask.clone())
        return v.clone() if torch.is_tensor(v) else v
    return {k: c(v) for k, v in samples.items()}, [{k: c(v) for k, v in t.items()} for t in targets]


def _copy_batch(dst_s, dst_t, samples, targets):
    if samples is dst_s and targets is dst_t:        # the caller filled the static buffers in place (CapturedTrainStep.batch)
        return
    dst, src = [], []
    for k, v in samples.items():
        if isinstance(v, utils.NestedTensor):
            dst += [dst_s[k].tensors, dst_s[k].mask]; src += [v.tensors, v.mask]
        elif torch.is_tensor(v):
            dst.append(dst_s[k]); src.append(v)
    for d, t in zip(dst_t, targets):
        for k, v in t.items():
            if torch.is_tensor(v):
                dst.append(d[k]); src.append(v)
    # device -> device with matching dtypes (the steady state of a loop: batches come from the prefetcher): ONE multi-tensor
    # copy for the ~20 small fields instead of a launch each -- they sit on the critical path between two replays
    big = [i for i, (a, b) in enumerate(zip(dst, src)) if a.numel() >= (1 << 20) or a.dtype != b.dtype or a.device != b.device
           or a.shape != b.shape]
    for i in big:
        dst[i].copy_(src[i], non_blocking=True)
    groups = {}
    for i in range(len(dst)):
        if i not in set(big):
            groups.setdefault(dst[i].dtype, []).append(i)
    for idx in groups.values():                       # one launch per dtype (the multi-tensor fast path wants uniform lists)
        torch._foreach_copy_([dst[i] for i in idx], [src[i] for i in idx], non_blocking=True)


# Stream capture is made thread-local: torch.distributed's RCCL watchdog thread polls hipEventQuery on its own schedule,
# which a process-global capture would turn into hipErrorStreamCaptureUnsupported (and an abort) at world_size > 1.
_CAPTURE_MODE = "thread_local"


@contextlib.contextmanager
def _capture(graph, **kw):
    """`torch.cuda.graph(...)` with Python's cyclic garbage collector switched OFF for the duration of the capture.  A step's capture
    runs ~1500 Python-level launches; a generation-2 collection in the middle of it can finalize an OLDER CapturedTrainStep (its graphs,
    its private pool, its events) -- device frees and graph destruction inside an open capture.  Seen in round 6 as `Fatal Python error:
    Aborted` with `Garbage-collecting` on the stack inside `flush_wgrads_side` during a capture, and as segfaults in later replays, once the
    GPU suite held enough dead captures; torch's own context collects BEFORE the capture but does not stop a collection during it."""
    import gc
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE, **kw):
            yield
    finally:
        if was:
            gc.enable()


def _warm_up(fn, n):
    """`fn` n times on a side stream before it is captured (operand refresh, workspaces, descriptor tables), joined and synchronized:
    no collective is in flight while capturing (see _CAPTURE_MODE)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


class CapturedTrainStep:
    """The loop body (engine_vg.py:40-72) captured into HIP graphs for one input shape.

    A step is 427 kernel launches; replaying them from a hipGraph removes the per-launch host cost.  Everything
    that changes from step to step lives in device memory (dropout step-seed word, optimizer step counter, the
    input batch copied into static buffers), so replays are real training steps.  With world_size > 1 the body is
    three graphs (forward + backward phase 1 | ResNet backward | clip + AdamW) around the two eager, asynchronous
    gradient exchanges of reftr_amd.parallel.DistributedDataParallel.  Shapes other than the captured one must use
    `train_step`.

    Single-process runs use the DEFERRED optimizer schedule (one graph): iteration i ends with the gradient norm, its
    AdamW update is applied at the head of iteration i+1 -- the ResNet / transformer slice first on the main stream, the
    BERT slice (72 % of the 4.25 GB pass) on the language stream in front of the BERT operand refresh, concurrently with
    the ResNet forward.  Same arithmetic, same order of updates; whoever reads the weights or the optimizer state in
    between (`model(...)` outside the replay, `state_dict()`, `optimizer.step()`) first gets the pending update applied
    (`flush()`).  The learning rates are device words (`optimizer.lr_dev`): the update of iteration i uses the rates that
    were current when iteration i ran, and schedule changes need no re-capture.

    `accumulate=True` (gradient accumulation, begin_train_step(accum_steps > 1)): the graph is forward + loss + backward ONLY -- no
    optimizer node of any kind, so no update can run between the micro-batches of a window.  The caller launches
    optimizer.accumulate(), or finish_accumulation() + clip + update, eagerly between replays.

    `canvas` (reftr_amd.data.canvas.BatchCanvas): the static buffers have the canvas's size and the criterion reads boxes, offsets,
    box count and target masks from device buffers (`criterion.targets_static`), all of them rewritten by ONE rt_batch_stage launch
    per batch -- so the one capture serves every batch that fits the canvas, whatever its image size, box counts and mask sizes.
    """

    def __init__(self, model, criterion, optimizer, max_norm, samples, targets, warmup=2, force_two_phase=False, force_phases=None,
                 accumulate=False, canvas=None):
        self.model, self.criterion, self.optimizer, self.max_norm = model, criterion, optimizer, max_norm
        self.accumulate = bool(accumulate)
        self.inner = _inner(model)
        self.ddp = model if model is not self.inner else None
        self.canvas, self.staged = canvas, None
        if canvas is None:
            self.s, self.t = _clone_batch(samples, targets)
            self.key = self.shape_key(samples, targets)
        else:
            assert self.ddp is None, "the canvas is a single-process schedule"
            if canvas.tokens is None:
                canvas.bind(samples)                 # the token field shapes of the capture: other lengths no longer fit
            self.staged = canvas.stage(samples, targets)              # fresh canvas-sized buffers, filled with this batch
            self.s, self.t = self.staged.samples, [{} for _ in targets]      # the criterion reads the staged targets alone
            self.key = canvas.key(samples)
        self._lrs = [g["lr"] for g in optimizer.param_groups]
        inner = self.inner
        # the cooperative decoder's failure word vetoes an iteration's update on the device and travels in the stats vector
        self.fail_word = inner.coop_failure_word() if hasattr(inner, "coop_failure_word") else None
        if hasattr(optimizer, "veto"):
            optimizer.veto = self.fail_word
        warmup = max(warmup, 2)          # the second step is the first one with the steady-state operand refresh
        # criterion.py:176-180 averages the box count over ranks: that collective runs eagerly before every replay and
        # the graph reads its result from a static device scalar
        self.nb = None
        if utils.is_dist_avail_and_initialized():
            self.nb = torch.zeros(1, dtype=torch.float32, device=self.s["sentence"].device)
            self._refresh_num_boxes(targets)
        # collectives stay outside the graphs: the engine calls the hooks between replays
        self._phase_hooks, self._post = inner._phase_hooks, inner._post_backward_hooks
        # data parallel: backward is captured as one graph per segment between the exchange points the wrapper registered
        # (RefTR.BOUNDARIES), so that each slice's all-reduce is issued the moment it is final and runs under the next graphs
        self.phases = [b for b in inner.active_boundaries() if self._phase_hooks.get(b)]
        if force_phases is not None:
            self.phases = [b for b in inner.active_boundaries() if b in force_phases]
        elif force_two_phase and not self.phases:
            # serial schedule: [everything but the ResNet | the ResNet]; interleaved: [... transformer backward | BERT || ResNet]
            self.phases = ["bert"] if inner.dp_schedule == "serial" else ["main"]
        self.two_phase = bool(self.phases)
        can_defer = hasattr(optimizer, "enable_deferred") and os.environ.get("REFTR_DEFER_OPT", "1") == "1"
        can_defer = can_defer and not self.accumulate
        self.deferred = can_defer and not self.two_phase and not self._post
        # data parallel: the same deferred schedule across the segment graphs -- the AdamW pass of iteration i sits at the head of
        # iteration i+1's FIRST graph (its BERT slice on the language stream under the ResNet forward, reading the all-reduced bf16
        # gradients of iteration i, which nothing rewrites before this iteration's first exchange boundary), the last graph ends
        # with the gradient norm.  (Optimizers without the deferred interface: clip + step in the last graph.)
        self.deferred_dp = can_defer and not self.deferred
        self._pending = False
        self._staged = None
        # a schedule is [head graph | per phase: its exchange hooks, then the segment graph that follows | tail graph]; tail None:
        # the head is the whole step
        if self.deferred:
            self._deferred_hooks()
            head, tail = self._step_deferred, None
        else:
            if hasattr(optimizer, "enable_device_lr") and not self.accumulate:
                optimizer.enable_device_lr()
            if self.deferred_dp:
                self._deferred_hooks()
                head, tail = self._head_deferred, self._tail_deferred
            elif self.accumulate:
                assert not self.phases and not self._post, "accumulation is a single-process schedule"
                # the stats vector is packed inside the graph, as _opt / _tail_deferred do; the optimizer's launches stay outside
                # it, and the window's norm is the eager clip's (_update)
                head, tail, self.grad_norm = self._fwd_bwd_stats, None, None
            else:
                head, tail = self._fwd_bwd, self._opt

        def iteration():
            head()
            for name in self.phases:
                self._run(self._phase_hooks.get(name, ()))
                inner.continue_backward()
            self._run(self._post)
            if tail is not None:
                tail()
        with self._building():
            _warm_up(iteration, warmup)
            self.g_fb = torch.cuda.CUDAGraph()
            with _capture(self.g_fb):
                self.out = head()
            self.g_seg = []
            for name in self.phases:                 # the segment that FOLLOWS boundary `name`
                g = torch.cuda.CUDAGraph()
                with _capture(g, pool=self.g_fb.pool()):
                    inner.continue_backward()
                self.g_seg.append(g)
            assert inner._bwd_gen is None, "backward did not run to its end during capture"
            self.g_bb = self.g_seg[-1] if self.g_seg else None
            self.g_opt = None
            if tail is not None:
                self.g_opt = torch.cuda.CUDAGraph()
                with _capture(self.g_opt, pool=self.g_fb.pool()):
                    tail()
            if self.deferred or self.deferred_dp:
                self.grad_norm = optimizer.grad_norm
                if self.deferred and getattr(optimizer, "_emit", False):
                    optimizer._emit_tables(None)       # flush() applies the update over the WHOLE buffer: its job / chunk tables are built
                                                       # now (a pageable host -> device copy later would stall the host behind queued work)
                self._pending = True                   # the last warm-up iteration's update
                self._set_flush(True)

    @contextlib.contextmanager
    def _building(self):
        """While this capture is warmed up and captured: the model's exchange hooks are parked (the capture calls them itself,
        between its graphs), backward stops at this schedule's phases, and the criterion reads the static box count and, on a canvas,
        the staged targets.  All of it is undone on the way out, also after an error."""
        inner, crit, st = self.inner, self.criterion, self.staged
        inner._phase_hooks, inner._post_backward_hooks = {}, []
        inner._stops = frozenset(self.phases)
        if self.nb is not None:
            crit.num_boxes_static = self.nb
        if st is not None:
            crit.targets_static, crit.target_masks_static = st.targets_static, st.tgt_masks
        try:
            yield
        finally:
            inner._phase_hooks, inner._post_backward_hooks = self._phase_hooks, self._post
            inner._stops = frozenset()
            crit.num_boxes_static = None
            if st is not None:
                crit.targets_static = crit.target_masks_static = None

    # ------------------------------------------------------------------ deferred optimizer schedule
    def _deferred_hooks(self):
        from .models import layout as L
        inner, opt = self.inner, self.optimizer
        opt.enable_deferred()
        bb, be = inner.store.group_range[L.GROUP_BERT]
        assert be == inner.store.flat_p.numel() or be > bb, "BERT is the last group of the flat buffers"
        self._hooks = ((lambda: opt.apply_pending(span=(0, bb)) if bb > 0 else None),
                       (lambda: opt.apply_pending(span=(bb, be))))

    def _head_deferred(self):
        """[AdamW of the previous iteration | forward | loss | backward up to the first boundary]"""
        inner = self.inner
        self._set_flush(False)
        inner._pre_update = self._hooks
        try:
            return self._fwd_bwd()
        finally:
            inner._pre_update = None

    def _tail_deferred(self):
        self.grad_norm = self.optimizer.finish_step(self.max_norm)
        self._pack_stats()

    def _set_flush(self, on):
        f = self.flush if on else None
        self.inner._flush_pending = f
        self.optimizer._flush_pending = f

    def _step_deferred(self):
        """[AdamW of the previous iteration | forward | loss | backward | gradient norm] -- eagerly or under capture."""
        inner, opt = self.inner, self.optimizer
        self._set_flush(False)
        inner._pre_update = self._hooks
        # (the gradient clear stays between loss and backward on the main stream: on the language stream under the encoder it was
        # neutral, 6.67-6.69 vs 6.66-6.68 ms, profiles/r04ai_zero_side_ab.txt and again +0.06 ms in round 5 -- option removed)
        # backward and clip norm are one unit here (nothing touches the gradient buffer in between): the BERT slice's share of the
        # norm may be taken on the language stream as soon as that slice is final (reftr_transformer._backward_gen)
        inner._norm_side = not getattr(inner.store, "fused_norm", False)
        try:
            out = self._fwd_bwd(zero=True)
            self.grad_norm = opt.finish_step(self.max_norm, loss=out[0], stats=self._stats_spec())
            from . import hip as _H
            _H.mark("gradient norm done (step end)")
        finally:
            inner._pre_update = None
            inner._norm_side = False
            inner._norm_split = None
        self._pack_stats()
        return out

    def flush(self):
        """Applies the pending update now (before an eager forward, a checkpoint, an optimizer.step())."""
        if not ((self.deferred or self.deferred_dp) and self._pending):
            return
        self._pending = False
        self._set_flush(False)
        emitted = self.optimizer.apply_pending()
        self.optimizer.clear_pending()
        if emitted:
            self.inner.operands_emitted()
        else:
            self.inner.mark_dirty()

    def reset_pending(self):
        """Forgets the pending update (after / before the caller restores weights / optimizer state by hand).  The bf16 operands are
        marked stale: the next replay rebuilds them from whatever the masters then hold (the graphs carry no operand refresh of
        their own since the optimizer's pass writes the operands)."""
        self._pending = False
        self.inner.mark_dirty()
        if self.deferred or self.deferred_dp:
            self.optimizer.clear_pending()
            self._set_flush(False)

    def _refresh_num_boxes(self, targets, reduced=None):
        if self.nb is None:
            return
        if reduced is not None:               # already averaged over the ranks by the iteration's capture decision (one collective)
            self.nb.copy_(reduced)
            return
        self.nb.fill_(float(sum(len(t["labels"]) for t in targets)))
        torch.distributed.all_reduce(self.nb)
        self.nb.div_(utils.get_world_size())

    @staticmethod
    def shape_key(samples, targets):
        # every tensor field of the targets is copied into the static batch (_copy_batch) and read by the criterion at its
        # captured shape: boxes, labels, masks (RefTRSeg), sizes ... all belong to the key
        return _sample_shapes(samples) + tuple(tuple((n, tuple(v.shape)) for n, v in sorted(t.items()) if torch.is_tensor(v))
                                               for t in targets)

    def _direct_loss_ok(self):
        """The direct loss path applies when the total is the weighted sum of the box losses of THIS process's model: no wrapper
        (the data-parallel schedules drive backward themselves), no mask / CEM terms, the fused total, aux weights as usual."""
        inner, crit = self.inner, self.criterion
        # (round 5 built this path under the data-parallel wrapper too and measured it through single-rank RCCL: 7.58-7.63 ms against
        # 7.17-7.22 ms on the autograd path -- the early fork of the target preparation costs the segment graphs more than the launches it
        # removes; profiles/r05_ddp_direct_loss_negative_result.txt.  Removed.)
        dp_ok = self.model is inner and not inner.dp_mode
        return (os.environ.get("REFTR_LOSS_DIRECT", "1") == "1" and dp_ok and getattr(inner, "seg", 1) is None
                and hasattr(crit, "loss_and_grad") and tuple(crit.losses) == ("boxes",)
                and os.environ.get("REFTR_FUSED_TOTAL", "1") != "0")

    def _fwd_bwd_direct(self, zero):
        inner, crit = self.inner, self.criterion
        dev = inner.store.device
        side = inner.net.side
        main = torch.cuda.current_stream()
        prepared = side.run(lambda: crit.prepare(self.t, dev))            # reads the targets only: beside the step head, not behind the forward
        # round 5: with the fused head (rt_head_loss) the forward itself ends with the losses and the head's backward-data; it needs
        # the prepared targets (ready at the forward join, where the side stream comes in)
        inner.__dict__["_head_fused"] = (crit, prepared) if os.environ.get("REFTR_HEAD_FUSE", "1") != "0" else None
        try:
            logits = inner(self.s, _logits_only=True)                      # joins the side stream at its forward join
        finally:
            inner.__dict__["_head_fused"] = None
        if side.enabled:
            for t in prepared:
                t.record_stream(main)
        head = inner._saved.get("head")
        if head is not None:
            box, dl = head["losses"], None                                 # backward starts behind the head (RefTR._backward_phases)
            loss_dict = crit._loss_dict(box)
            losses = head["total"][0]                                      # the weighted total (engine_vg.py:43), from the same launch
        else:
            loss_dict, box, dl = crit.loss_and_grad(logits, inner._saved["phrase_mask"], prepared, inner.aux_loss)
            # the weighted total is only logged (engine_vg.py:43,46-53): the same two torch kernels as in the autograd path.  On the
            # main stream: forked to the side stream here (measured) the replayed graph's whole backward slows down by 0.25 ms
            losses = crit.weighted_total(loss_dict)
        if zero:
            _zero_grad(self.optimizer)
        inner._backward_impl(dl)                                           # ends with the side stream joined
        self._last = (losses.detach(), {k: v.detach() for k, v in loss_dict.items()})
        return self._last

    def _fwd_bwd(self, zero=True):
        if self._direct_loss_ok():
            return self._fwd_bwd_direct(zero)
        outputs = self.model(self.s)
        loss_dict = self.criterion(outputs, self.t)
        losses = _total(self.criterion, loss_dict)
        if zero:
            _zero_grad(self.optimizer)
        losses.backward()
        self._last = (losses.detach(), {k: v.detach() for k, v in loss_dict.items()})
        return self._last

    def _fwd_bwd_stats(self):
        """The whole graph of an accumulating capture: forward + loss + backward, then the losses packed for the host."""
        out = self._fwd_bwd()
        self._pack_stats()
        return out

    def _stats_spec(self):
        """The stats vector as rt_finish_stats writes it (deferred single-process schedule): (loss scalars sorted by name, whether the
        failure word rides along, the static output vector) -- or None when a loss is not an fp32 device scalar (then _pack_stats)."""
        ld = self._last[1]
        names = tuple(sorted(ld))
        srcs = [ld[k].reshape(1) for k in names]
        if len(srcs) > 40 or any(not (t.is_cuda and t.dtype == torch.float32) for t in srcs):
            self._stats_fused = False
            return None
        n = len(srcs) + (1 if self.fail_word is not None else 0) + 1
        if getattr(self, "stats", None) is None or self.stats.numel() != n or not self.stats.is_cuda:
            self.stats = torch.empty(n, dtype=torch.float32, device=srcs[0].device)
        self.stat_names = names
        self._stats_fused = True
        return srcs, self.fail_word is not None, self.stats

    def _pack_stats(self):
        """Every scalar the loop reads from an iteration -- the unweighted losses (sorted by name) and the gradient norm -- in
        ONE static device vector (a single small kernel at the end of the graph): the engine fetches it with one device -> host
        copy per iteration instead of one .item() per meter (the reference: engine_vg.py:46-53,69-72, util/misc.py:156-160)."""
        if getattr(self, "_stats_fused", False):      # rt_finish_stats wrote them (this iteration's finish_step)
            self._stats_fused = False
            return
        ld = self._last[1]
        self.stat_names = tuple(sorted(ld))
        # layout: [losses (sorted by name) | cooperative-launch failure word (when the model can raise one) | gradient norm]
        # (an accumulating capture has no norm of its own: its graph ends with the backward)
        fw = [self.fail_word.reshape(()).float()] if self.fail_word is not None else []
        gn = [self.grad_norm.reshape(()).float()] if self.grad_norm is not None else []
        self.stats = torch.stack([ld[k].reshape(()).float() for k in self.stat_names] + fw + gn)

    def queue_stats(self, stats=None):
        """Enqueues the device -> host copy of this iteration's stats vector behind the replay, into one of TWO pinned buffers used
        in turn (each with its event): a caller may launch iteration i + 1 before it reads iteration i, so the two
        copies in flight must not share a buffer.  Returns (host buffer, event)."""
        stats = self.stats if stats is None else stats
        if getattr(self, "_stats_host", None) is None:
            self._stats_host = [torch.empty(stats.numel(), dtype=torch.float32).pin_memory() for _ in range(2)]
            self._stats_event = [torch.cuda.Event(), torch.cuda.Event()]
            self._stats_flip = 0
        i = self._stats_flip
        self._stats_flip ^= 1
        self._stats_host[i].copy_(stats, non_blocking=True)
        self._stats_event[i].record()
        return self._stats_host[i], self._stats_event[i]

    @staticmethod
    def _run(hooks):
        for h in hooks:
            h()

    def _opt(self):
        self.grad_norm = self.optimizer.clip_grad_norm_(self.max_norm)
        self.optimizer.step()
        self._pack_stats()

    @property
    def batch(self):
        """The static input buffers the graphs read: (samples, targets).  An input pipeline that writes the next batch INTO
        them (reftr_amd.data's device kernels take an output tensor) and calls `step(*step.batch)` pays no staging copy;
        any other batch of the captured shape is copied in (one small copy per field) before the replay."""
        return self.s, self.t

    def accepts(self, samples, targets):
        """Whether this capture can replay the batch: its shape key -- or, on a canvas, any batch that fits."""
        if self.canvas is not None:
            return self.canvas.key(samples) == self.key and self.canvas.fits(samples, targets)
        return self.shape_key(samples, targets) == self.key

    def _fill(self, samples, targets):
        """The batch into the static buffers: the grouped copy, or on a canvas one rt_batch_stage launch for image, padding mask,
        boxes, offsets, box count and target masks plus the grouped copy for the fixed-shape token fields."""
        if self.canvas is None:
            return _copy_batch(self.s, self.t, samples, targets)
        if samples is self.s:
            return
        self.canvas.stage(samples, targets, out=self.staged, tokens=False)
        _copy_batch(self.s, [], {k: v for k, v in samples.items() if k != "img"}, [])

    def stage(self, samples, targets):
        """Copies the NEXT batch into the static input buffers now -- stream-ordered behind the replay that is still running,
        while the host would otherwise idle in front of the iteration's device -> host copy -- so that the next call only has to
        launch the graph.  Returns False (and does nothing) for a batch of another shape."""
        if samples is None or not self.accepts(samples, targets):
            return False
        self._fill(samples, targets)
        self._staged = (samples, targets)
        return True

    def _stage_in(self, samples, targets):
        staged, self._staged = self._staged, None
        if staged is None or staged[0] is not samples or staged[1] is not targets:
            self._fill(samples, targets)

    def __call__(self, samples, targets, nb_reduced=None):
        staged = self._staged is not None and self._staged[0] is samples and self._staged[1] is targets
        assert staged or (samples is self.s and targets is self.t) or self.accepts(samples, targets), \
            "captured for another input shape; use train_step"
        if self.inner._operands_dirty:        # the masters were changed outside an optimizer step (load_state_dict, a restored
            self.inner.refresh_now()          # snapshot): the graph no longer carries an operand refresh of its own
        if hasattr(self.optimizer, "check_sparse_state"):
            self.optimizer.check_sparse_state()      # moments restored from outside: the sparse-state bytes go back to 'unknown'
        if self.accumulate:
            self._stage_in(samples, targets)
            self.g_fb.replay()                # forward + loss + backward; what happens to the gradients is the caller's next launch
            # the replayed backward cleared and refilled the clip-norm accumulator like an eager one (zero_for_backward): say so on the
            # host, where that bookkeeping only ran at capture time
            st = self.inner.store
            st.norm_valid = bool(getattr(st, "fused_norm", False))
            self.inner._norm_split = None
            return self.out[0], self.out[1], None
        if self.deferred:
            self._stage_in(samples, targets)
            self.g_fb.replay()                # applies iteration i-1's update with the rates synced at iteration i-1
            self._sync_lr_if_changed()        # this iteration's rates, for the update the NEXT replay (or flush) applies
            self.optimizer.step_count += 1
            self._pending = True
            self._set_flush(True)
            return self.out[0], self.out[1], self.grad_norm
        if not self.deferred_dp:
            self._sync_lr_if_changed()        # stream-ordered, in front of this iteration's optimizer graph
        self._stage_in(samples, targets)
        self._refresh_num_boxes(targets, reduced=nb_reduced)
        self.g_fb.replay()                # deferred: applies iteration i-1's update with the rates synced at iteration i-1
        if self.deferred_dp:
            self._sync_lr_if_changed()    # this iteration's rates, for the update the NEXT replay (or flush) applies
        for name, g in zip(self.phases, self.g_seg):
            self._run(self._phase_hooks.get(name, ()))       # this slice is final: its all-reduce goes out now ...
            g.replay()                                       # ... and runs under the next segment of backward
        self._run(self._post)
        self.g_opt.replay()
        self.optimizer.step_count += 1
        if self.deferred_dp:
            self._pending = True
            self._set_flush(True)
        elif not getattr(self.optimizer, "_last_emitted", False):
            self.inner.mark_dirty()      # eager forwards after a replay must rebuild the bf16 operands
        return self.out[0], self.out[1], self.grad_norm

    def _sync_lr_if_changed(self):
        """The param groups' learning rates to the device words the optimizer's launches read, when the schedule moved them since
        the last call; an optimizer without device rates has its graph captured again."""
        lrs = [g["lr"] for g in self.optimizer.param_groups]
        if lrs == self._lrs:
            return
        if getattr(self.optimizer, "lr_dev", None) is not None:
            self._lrs = lrs
            self.optimizer.sync_lr()
        else:
            self.refresh_lr()

    def refresh_lr(self):
        self._lrs = [g["lr"] for g in self.optimizer.param_groups]
        self.g_opt = torch.cuda.CUDAGraph()
        sc = self.optimizer.step_count
        with _capture(self.g_opt, pool=self.g_fb.pool()):
            self._opt()
        self.optimizer.step_count = sc


def dp_capture_decision(can_replay, can_capture, device, num_boxes=None):
    """The collective choice between replaying, capturing and the eager loop body under data parallelism: 'replay' only if
    EVERY rank can replay its batch, 'capture' only if every rank would capture, else 'eager' on every rank.  ONE all-reduce per
    iteration: with `num_boxes` (this rank's box count) the same collective also carries the criterion's box-count average
    (criterion.py:176-180), which a replay would otherwise have to all-reduce on its own right behind this one -- returns
    (decision, device tensor [1] = world-average box count) then, the decision alone otherwise."""
    v = torch.tensor([0.0 if can_replay else 1.0, 0.0 if can_capture else 1.0, float(num_boxes or 0.0)], dtype=torch.float32, device=device)
    torch.distributed.all_reduce(v)                       # SUM: a rank that cannot contributes 1
    no_replay, no_capture, _ = v.tolist()
    decision = "replay" if no_replay == 0 else ("capture" if no_capture == 0 else "eager")
    if num_boxes is None:
        return decision
    return decision, v[2:3] / utils.get_world_size()


class Lookahead:
    """The next batch of a loop, fetched at most once: by the step while the device is busy with the current batch (the
    captured path calls it between the graph launch and the iteration's host sync), else by the loop itself."""

    def __init__(self, fn):
        self.fn, self.batch, self.done = fn, None, False

    def __call__(self):
        if not self.done:
            self.batch, self.done = self.fn(), True
        return self.batch


class _EagerResult:
    """finish() of a step that ran eagerly: the values are already there."""

    def __init__(self, res):
        self.res = res

    def finish(self):
        return self.res


def _read_stats(cap, criterion, slot, retry):
    """The host read-out of a replayed iteration: waits for the stats copy and returns (host vector, (loss_value, scaled dict,
    unscaled dict)).  A raised cooperative-decoder failure word re-runs the iteration instead -- (None, what `retry` returned) --
    and a non-finite loss stops the run (engine_vg.py:55-58)."""
    host_buf, event = slot
    event.synchronize()
    host = host_buf.tolist()
    k = len(cap.stat_names)
    if cap.fail_word is not None and host[k] != 0:
        # A stage hand-off of the cooperative decoder launches timed out in this iteration (under data parallelism: on any
        # rank -- the word was summed with the losses).  Its AdamW update was never armed (optimizer.finish_step's device-side
        # veto; an accumulating micro-batch has not reached the accumulator yet), so no parameter has changed; the launches are
        # switched off, the captures dropped, and the SAME batch is run again on the launched chain with the dropout seeds and
        # learning rates it had.
        if retry is None:
            _coop_fallback(cap.model)
            raise RuntimeError("rt_decoder_fwd: a stage hand-off timed out and the iteration cannot be re-run from here "
                               "(replayed without begin_train_step); the launches are now off (REFTR_DEC_COOP=0)")
        return None, retry()
    return host, _read_out(dict(zip(cap.stat_names, host)), criterion.weight_dict)


class _ReplayInFlight:
    """A replayed step between its launch and its host read-out (`finish`).  `then` is what follows the read-out and yields the
    gradient norm: nothing for the plain step, whose norm is the last word of the stats vector; for a micro-batch of an accumulation
    window `_update` -- its losses are read first, so the non-finite stop and the cooperative decoder's re-run come BEFORE
    its gradients go anywhere, as in the eager loop body."""

    def __init__(self, cap, criterion, retry=None, slot=None, then=None):
        self.cap, self.criterion, self.retry, self.then = cap, criterion, retry, then
        self.slot = slot if slot is not None else (cap._stats_host[0], cap._stats_event[0])

    def finish(self):
        host, res = _read_stats(self.cap, self.criterion, self.slot, self.retry)
        if host is None:
            return res
        return (*res, host[-1] if self.then is None else self.then())


def _new_capture(model, criterion, optimizer, max_norm, samples, targets, accumulate, canvas):
    """A CapturedTrainStep for this batch, with what its warm-up iterations moved taken back, so that the loop sees exactly one
    update per batch, like the eager loop.  The plain step's warm-up iterations are real updates on this batch: weights, both
    moments, the step counters and the dropout seed go back.  An accumulating capture's are forward + backward only: no weight or
    optimizer state moves, but the dropout seed does."""
    inner = _inner(model)
    st = inner.store
    seed = (inner.seed_dev.clone(), inner._step)
    snap = None if accumulate else (st.flat_p.clone(), optimizer.m.clone(), optimizer.v.clone(), optimizer.step_dev.clone(),
                                    optimizer.step_count)
    cap = CapturedTrainStep(model, criterion, optimizer, max_norm, samples, targets, accumulate=accumulate, canvas=canvas)
    cap.training = model.training
    if snap is not None:
        cap.reset_pending()
        st.flat_p.copy_(snap[0]); optimizer.m.copy_(snap[1]); optimizer.v.copy_(snap[2]); optimizer.step_dev.copy_(snap[3])
        optimizer.step_count = snap[4]
    inner.seed_dev.copy_(seed[0]); inner._step = seed[1]
    if snap is not None:
        inner.mark_dirty(full=True)      # the replay's first act finds the operands dirty and rebuilds them from the restored masters
    return cap


def _find_capture(model, criterion, samples, targets, optimizer, max_norm, max_shapes, canvas, accumulate):
    """How this batch runs, and on what: ("staged" | "replay" | "capture" | "eager", the CapturedTrainStep or None, the canvas if
    the batch goes through it, the world-average box count if the data-parallel decision already carries it).  The captures live
    in `model._captured_steps`, keyed by (shape key or canvas key, criterion, optimizer, max_norm or "accumulate", training)."""
    state = _state(model)
    dist_on = _multi_rank()
    cap = state.staged_cap
    if cap is not None and not dist_on and cap._staged is not None and cap._staged[0] is samples and cap._staged[1] is targets \
            and cap.criterion is criterion and cap.optimizer is optimizer and cap.max_norm == max_norm and cap.training == model.training \
            and cap.canvas is canvas and not accumulate:
        return "staged", cap, canvas, None                     # steady state: staged by the previous iteration's lookahead
    state.staged_cap = None
    inner = _inner(model)
    caps = inner.__dict__.setdefault("_captured_steps", {})
    ok = _on_device(samples) and os.environ.get("REFTR_TRAIN_GRAPH", "1") == "1"
    if accumulate:                                    # (the caller has checked _require_accumulation)
        ok = ok and not dist_on and model is inner
    else:
        ok = ok and hasattr(optimizer, "clip_grad_norm_")
    if canvas is not None and not _canvas_fits(model, canvas, samples, targets):
        canvas = None                                 # the existing path, at the batch's own shape
    key = None
    if ok:
        skey = canvas.key(samples) if canvas is not None else CapturedTrainStep.shape_key(samples, targets)
        key = (skey, id(criterion), id(optimizer), "accumulate" if accumulate else float(max_norm), model.training)
        ok = key in caps or len(caps) < max_shapes
    nb_reduced = None
    if dist_on and not accumulate:
        # Data parallel: replaying, capturing and the eager loop issue DIFFERENT collective sequences (a capture adds the
        # num_boxes all-reduce of its constructor and warm-up iterations with real gradient exchanges), and both the shape
        # key (per-image box counts, image sizes) and the capture budget are rank-local.  The choice is therefore made
        # collectively: replay only if EVERY rank holds a capture for its batch, capture only if every rank would capture,
        # otherwise every rank runs the eager step.  One 3-word all-reduce per iteration, issued while the device is
        # idle behind the previous iteration's read-out.
        mine = ok
        decision, nb_reduced = dp_capture_decision(ok and key in caps, ok and key not in caps, inner.store.device,
                                                   num_boxes=sum(len(t["labels"]) for t in targets))
        ok = decision != "eager"
        if decision != "replay":
            nb_reduced = None                   # the capture / eager paths reduce the box count themselves
        if mine and not ok:
            # this rank could have replayed / captured, another one could not (its capture budget is spent, or its batch has a
            # shape this rank already holds while the other must still capture): the whole job runs this iteration eagerly.
            # Said once per shape -- a run that quietly degrades to eager launches is 2-3x slower.
            _say_once(model, ("dp", key), f"[reftr_amd] rank {utils.get_rank()}: data-parallel step runs eagerly (ranks disagree on "
                      f"replay/capture for this input shape; {len(caps)} of {max_shapes} captures in use)")
    cap = caps.get(key) if ok else None
    # one pending (deferred) update at a time, and it lands before anything else runs -- an eager forward, a capture's warm-up,
    # another capture's replay: every capture but the one about to replay is flushed
    for other in caps.values():
        if other is not cap:
            other.flush()
    if not ok:
        return "eager", None, canvas, None
    if cap is not None:
        return "replay", cap, canvas, nb_reduced
    cap = caps[key] = _new_capture(model, criterion, optimizer, max_norm, samples, targets, accumulate, canvas)
    return "capture", cap, canvas, None


@contextlib.contextmanager
def _update_rewound(optimizer, lrs):
    """Around the re-run of a replayed plain step whose update was vetoed: what the failed iteration advanced goes back -- the host
    step count and, while the re-run lasts, the learning rates it ran with (its scheduler step has already happened)."""
    optimizer.step_count -= 1
    # The veto is a per-rank device word, the decision to run the iteration again is collective: a healthy rank's finish_step
    # has advanced its device counter, the failing rank's was vetoed.  Every rank re-bases the device counter on the host count
    # (the same on all ranks), otherwise the AdamW bias corrections of the replicas differ from here on.
    optimizer.step_dev.fill_(optimizer.step_count)
    after = [g["lr"] for g in optimizer.param_groups]
    for g, lr in zip(optimizer.param_groups, lrs):
        g["lr"] = lr
    try:
        yield
    finally:
        for g, lr in zip(optimizer.param_groups, after):
            g["lr"] = lr


def begin_train_step(model, criterion, samples, targets, optimizer, lr_scheduler=None, max_norm=0.0, max_shapes=4, lookahead=None,
                     accum_steps=1, window_end=None, canvas=None):
    """Launches one iteration of the loop body and returns a handle; `handle.finish()` waits for it and returns what
    `train_step` returns.  Between the two the caller may do host work (the epoch loop books the previous iteration's meters).

    Replayed from hipGraphs: the first batch of an input shape captures a CapturedTrainStep (kept on the model), later batches
    of that shape replay it; CPU tensors, foreign optimizers and more than `max_shapes` different shapes (variable-size data)
    run the eager `train_step`.  `lookahead` (a Lookahead) is called while the replay runs: the next batch is fetched and staged
    into the graph's input buffers under the current step instead of in front of the next one.

    Everything the host does between an iteration's read-out and the next launch is device idle time, so the steady state is
    short: a batch that the previous iteration already staged is recognised by identity (no shape key, no lookups), the
    scheduler step and the stats copy are issued right behind the launch.

    accum_steps > 1 (see train_step): one micro-batch of an accumulation window.  The replayed graph is forward + loss + backward
    alone (CapturedTrainStep(accumulate=True)); `finish` reads the losses and then launches accumulate() -- or, for the window's
    last micro-batch, the average, the clip, the update and the scheduler step -- eagerly, so the update of a window is applied at
    its end and never between two of its micro-batches.

    canvas (reftr_amd.data.canvas.BatchCanvas; single process): every batch that fits the canvas is staged into ONE capture's
    canvas-sized buffers by one rt_batch_stage launch and replayed -- the capture key is the canvas, the batch size and the token field
    shapes, not the batch's own shape.  A batch that does not fit runs exactly as without a canvas (own shape, `max_shapes`)."""
    if canvas is not None:
        _canvas_single_process(model)                 # refused before anything is launched
    accum_steps = int(accum_steps)
    accumulate = accum_steps > 1
    if accumulate:
        _require_accumulation(optimizer)
    samples, targets, canvas = _raw_batch(model, canvas, samples, targets)
    how, cap, on_canvas, nb_reduced = _find_capture(model, criterion, samples, targets, optimizer, max_norm, max_shapes, canvas, accumulate)
    if how == "eager":
        return _EagerResult(train_step(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, accum_steps, window_end,
                                       canvas=on_canvas))
    last = _window_last(optimizer, accum_steps, window_end) if accumulate else None
    lrs_now = [g["lr"] for g in optimizer.param_groups]
    seed_back = (1 if model.training else 0, 1)
    cap(samples, targets, nb_reduced)
    # ONE device -> host copy for everything the loop looks at (losses for the meters and the finite check, gradient norm);
    # under data parallelism the loss entries are first averaged over the ranks in one all-reduce (util/misc.py:136-160).
    # The copy is enqueued right behind the replay, into pinned memory; the host then spends the step's run time on the
    # scheduler, on fetching and staging the NEXT batch (H2D hand-over, copies into the graph's input buffers -- stream-ordered
    # BEHIND the stats copy) and only then waits for the copy's event.
    stats = cap.stats
    if _multi_rank():
        k = len(cap.stat_names)
        kf = k + (1 if cap.fail_word is not None else 0)      # the failure word rides along: SUM over ranks, non-zero = some rank failed
        stats = stats.clone()
        torch.distributed.all_reduce(stats[:kf])
        stats[:k] /= utils.get_world_size()
    slot = cap.queue_stats(stats)
    if lr_scheduler is not None and not accumulate:
        lr_scheduler.step()          # host state only; the device reads the new rates when the next launch syncs them
    state = _state(model)
    state.staged_cap = None
    if lookahead is not None:
        nxt = lookahead()
        if nxt is not None and nxt[0] is not None and cap.stage(*nxt) and not accumulate:
            state.staged_cap = cap           # (the identity fast path is the plain step's: a micro-batch always flushes the others)

    def _retry():
        # Nothing of the failed iteration has reached the weights (the device-side veto) or, for a micro-batch, the accumulator and
        # the scheduler: the same call again, without lookahead, on the launched chain and the dropout seeds it had.  The plain
        # step has already counted the update and stepped the scheduler: both are rewound around the re-run.
        _coop_fallback(model)
        with contextlib.nullcontext() if accumulate else _update_rewound(optimizer, lrs_now):
            _restore_seed(model, seed_back)
            return begin_train_step(model, criterion, samples, targets, optimizer, lr_scheduler if accumulate else None, max_norm,
                                    max_shapes, None, accum_steps, last, canvas).finish()
    # a micro-batch's graph ends with the backward: what follows it is launched eagerly behind the read-out
    then = (lambda: _update(model, optimizer, lr_scheduler, max_norm, last, sync_lr=True)) if accumulate else None
    return _ReplayInFlight(cap, criterion, retry=_retry, slot=slot, then=then)


def captured_train_step(model, criterion, samples, targets, optimizer, lr_scheduler=None, max_norm=0.0, max_shapes=4, lookahead=None,
                        accum_steps=1, window_end=None, canvas=None):
    """`train_step` with the same return value, on `begin_train_step` (launch) + `finish` (read-out)."""
    return begin_train_step(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, max_shapes, lookahead,
                            accum_steps, window_end, canvas).finish()


def _check_cooperative(model):
    """rt_decoder_fwd reports a consumer that gave up waiting (a workgroup that never became resident) through a device word;
    a loop that produced numbers from such a launch must not return them."""
    dc = getattr(getattr(_inner(model), "net", None), "dec_counters", None)
    if dc is not None and int(dc[-1]) != 0:
        raise RuntimeError("rt_decoder_fwd: a stage hand-off timed out (workgroups not co-resident?) -- set REFTR_DEC_COOP=0")


def train_one_epoch(model, criterion, data_loader, optimizer, lr_scheduler, device, epoch, max_norm=0, accum_steps=1, canvas=None):
    """engine_vg.py:22-79.  accum_steps = k > 1: every k batches of the loader form one accumulation window -- one clip, one update
    and one lr_scheduler.step() per window, on the mean of its gradients (see train_step).  The last window of an epoch may be cut
    short: it is finished with the r < k batches it has (s = 1 / r); no batch is dropped and nothing is carried into the next epoch.
    The stats board receives one row per micro-batch (its loss terms and the learning rate); `grad_norm` -- the norm of the window's
    averaged gradient -- is booked once per window, on the row of its last micro-batch.
    canvas (reftr_amd.data.canvas.BatchCanvas, e.g. BatchCanvas.from_args(args, first_samples)): variable-shape data -- per-batch
    image padding, ragged box counts, per-image mask sizes -- replayed from ONE capture (see begin_train_step)."""
    accum_steps = int(accum_steps)
    if canvas is not None:
        _canvas_single_process(model)
    if accum_steps > 1:
        _require_accumulation(optimizer)
        optimizer.accum_count = 0                 # a window never spans two epochs
    n_batches = len(data_loader)
    model.train()
    criterion.train()
    board = utils.StatBoard()
    header = "Epoch: [{}]".format(epoch)
    prefetcher = data_prefetcher(data_loader, device, prefetch=True)
    samples, targets = prefetcher.next()
    booked = None
    # The loop reads iteration i before it launches iteration i + 1 (engine_vg.py:53-58 stops on a non-finite loss BEFORE the update).
    # Launching i + 1 first was built in round 5 on the device-side veto that is still there (rt_finish_step never arms the update of
    # an iteration whose total is not finite) and measured SLOWER: a hipGraph launched while its previous launch is still running
    # starts later than one launched from an idle stream on this stack (+0.03 ... 0.11 ms per iteration, also with two instantiated
    # graphs used in turn; profiles/r05_pipeline_negative_result.txt).  Removed.

    def _read(step):
        loss_value, scaled, unscaled, gnorm = step.finish()
        if torch.is_tensor(gnorm):               # the eager step hands back the optimizer's device scalar, which the next step overwrites
            gnorm = float(gnorm)
        # what the reference's meter shows: the rate after this iteration's scheduler step (a window's last micro-batch steps it in finish)
        row = dict(loss=loss_value, **scaled, **unscaled, lr=optimizer.param_groups[0]["lr"] if accum_steps > 1 else step.lr_logged)
        if gnorm is not None:                    # (a micro-batch inside an accumulation window has none)
            row["grad_norm"] = gnorm
        return row

    for it in board.log_every(range(n_batches), 50, header):
        # the loop body of engine_vg.py:40-72 -- replayed from hipGraphs for fixed-shape data (RefCOCO: 640 x 640, L = 40), or, with a
        # canvas, for every batch that fits it;
        # the replayed path hands back host numbers (one stacked copy per iteration), the eager one device scalars.
        ahead = Lookahead(prefetcher.next)
        # (window_end is only read when accum_steps > 1)
        step = begin_train_step(model, criterion, samples, targets, optimizer, lr_scheduler, max_norm, lookahead=ahead,
                                accum_steps=accum_steps, window_end=(it + 1) % accum_steps == 0 or it + 1 == n_batches, canvas=canvas)
        step.lr_logged = optimizer.param_groups[0]["lr"]      # what the reference's meter shows: the rate after this iteration's scheduler step
        if booked is not None:
            board.add(**booked)
            booked = None
        booked = _read(step)
        samples, targets = ahead()
    if booked is not None:
        board.add(**booked)
    _check_cooperative(model)
    board.synchronize_between_processes()
    print("Averaged stats:", board)
    return board.global_avg()


class CapturedForward:
    """Inference forward replayed from one hipGraph per input shape (RefCOCO-style evaluation pads every image to the same
    square, datasets/transforms.py: NormalizeAndPad): ~600 launches become one replay.  The forward has no atomics, so the
    replayed outputs are bit-identical to the eager ones (tests/test_model_gpu.py).  Outputs are static buffers that the
    next replay overwrites."""

    def __init__(self, model, max_shapes=4):
        self.model, self.graphs, self.max_shapes = model, {}, max_shapes
        self._gen = _state(model).coop_generation

    shape_key = staticmethod(_sample_shapes)

    @torch.no_grad()
    def __call__(self, samples):
        if not isinstance(samples.get("img"), utils.NestedTensor):
            return self.model(samples)
        gen = _state(self.model).coop_generation
        if gen != self._gen:                     # the cooperative launches were switched off: the graphs that contain them go
            self.graphs, self._gen = {}, gen
        key = self.shape_key(samples)
        ent = self.graphs.get(key)
        if ent is None and len(self.graphs) >= self.max_shapes:      # variable-size data: eager launches
            return self.model(samples)
        if ent is None:
            s, _ = _clone_batch(samples, [])
            _warm_up(lambda: self.model(s), 1)
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                out = self.model(s)
            ent = self.graphs[key] = (g, s, out)
        g, s, out = ent
        _before_forward_replay(_inner(self.model))
        _copy_batch(s, [], samples, [])
        g.replay()
        return out


def _before_forward_replay(inner):
    """Before a captured forward is replayed: a pending deferred update is applied and dirty operands are rebuilt (the graph has no refresh)."""
    if inner._flush_pending is not None:
        inner._flush_pending()
    if inner._operands_dirty:
        inner.refresh_now()


class _ForwardLosses:
    """fwd(samples) -> criterion -> utils.reduce_dict -> one iteration's loss meters as ONE device vector, [unscaled..., scaled...,
    total] (no .item() per loss): (outputs, names, vector).  Keeps the weights on the device, renewed when the loss names change."""

    def __init__(self, fwd, criterion):
        self.fwd, self.criterion, self._wvec = fwd, criterion, None

    def __call__(self, samples, targets):
        outputs = self.fwd(samples)
        red, weight_dict = utils.reduce_dict(self.criterion(outputs, targets)), self.criterion.weight_dict
        names = sorted(red)
        wn = [k for k in names if k in weight_dict]
        if self._wvec is None or self._wvec[0] != names:
            self._wvec = (names, torch.tensor([weight_dict[k] for k in wn], dtype=torch.float32, device=red[names[0]].device))
        un = torch.stack([red[k].reshape(()).float() for k in names])
        sc = torch.stack([red[k].reshape(()).float() for k in wn]) * self._wvec[1]
        return outputs, [_UNSCALED(k) for k in names] + wn + ["loss"], torch.cat([un, sc, sc.sum().reshape(1)])


class CapturedEvalStep:
    """One evaluation batch on a batch canvas (reftr_amd.data.canvas) as ONE replay of ONE hipGraph: forward -> criterion (reading
    the staged targets, as CapturedTrainStep's canvas form does) -> the loss vector -> rt_eval_canvas (box selection and scaling,
    mask decisions from the logits, metrics, running totals, the batch's slot of the results ring).  Owns the StagedBatch, the
    per-image facts and the graph; the accumulators and the ring (`state`, a hip.EvalCanvasState) are handed in and outlive it.
    Per batch the host issues rt_batch_stage, rt_eval_facts and the grouped token copy and replays; nothing is copied back.

    The RAW form (the capture was built from a raw batch, reftr_amd.data.raw): the stage is rt_raw_stage, the facts come from host
    values by value (rt_eval_raw_facts: the resized sizes are RawImages.out_sizes(), the original sizes the raw images' own; `host_ids`:
    the image ids as python ints, None: gathered on the device from the targets' tensors) and, with a 'segm' post-processor, the tail
    ends with rt_eval_orig -- the mask scored once more on the raw frame against the raw annotation, into `acc_orig`.  The graph reads
    the raw masks through a table of their addresses: the step holds the batch's mask tensors until its next call.

    The cooperative decoder's fail-safe: the graph's metric launch takes the decoder's failure word as its veto, so the device tests
    the flag BEFORE the batch's results are kept -- a batch whose hand-off timed out leaves totals, ring and cursor untouched; the
    host reads the word as on every path (one 4-byte read per batch, only while cooperative launches are in use: _CanvasEval)."""

    def __init__(self, model, criterion, postprocessors, canvas, samples, targets, acc, slots, state=None, acc_orig=None, host_ids=None):
        self.model, self.criterion, self.canvas, self.inner = model, criterion, canvas, _inner(model)
        self.segm, self.raw = postprocessors.get("segm"), _is_raw(samples)
        if canvas.tokens is None:
            canvas.bind(samples)
        self.key = canvas.key(samples)
        self.staged = canvas.stage(samples, targets)              # fresh canvas-sized buffers, filled with this batch
        self.s, self.t = self.staged.samples, [{} for _ in targets]
        B, dev = len(targets), self.s["img"].tensors.device
        self.facts = torch.zeros((B, 6), dtype=torch.int32, device=dev)
        self.image_ids = torch.zeros(B, dtype=torch.int64, device=dev)
        # the raw form scores masks on the original frame too; every raw batch that fits the canvas has at most this many pixels
        self.max_pixels = H.RAW_STAGE_MAX_SCALE ** 2 * canvas.height * canvas.width
        self.orig = H.EvalOrigState(B, self.max_pixels, dev, acc=acc_orig) if self.raw and self.segm is not None else None
        self._keep = None
        self._gather_facts(samples, targets, host_ids)
        self.losses = _ForwardLosses(model, criterion)       # held with the graph: the replay reads the weight vector it keeps
        self._gen = _state(model).coop_generation    # a cooperative fall-back anywhere drops this capture: it contains the launches
        with self._building():
            warm = []
            _warm_up(lambda: warm.append(self.losses(self.s, self.t)), 1)
            P = int(warm[0][0]["pred_boxes"].shape[1])
            self.state = state if state is not None else H.EvalCanvasState(slots, B, P, dev, acc=acc)
            assert self.state.B == B and self.state.P == P
            # read after the warm-up: the hand-off buffer exists by now (None: no cooperative launches in this configuration)
            self.fail_word = self.inner.coop_failure_word() if hasattr(self.inner, "coop_failure_word") else None
            del warm
            self.graph = torch.cuda.CUDAGraph()
            with _capture(self.graph):
                outputs, self.names, self.vec = self.losses(self.s, self.t)
                self.last = self._tail(outputs)
            self.outputs = outputs

    @contextlib.contextmanager
    def _building(self):
        crit, st = self.criterion, self.staged
        crit.targets_static, crit.target_masks_static = st.targets_static, st.tgt_masks
        try:
            yield
        finally:
            crit.targets_static = crit.target_masks_static = None

    def _gather_facts(self, samples, targets, host_ids=None):
        if self.raw:
            return self._raw_facts(samples["img"], targets, host_ids)
        origs = [t["orig_size"] for t in targets] if "orig_size" in targets[0] else None
        ids = [t["image_id"] for t in targets] if "image_id" in targets[0] else None
        hw = [tuple(t["masks"].shape[-2:]) for t in targets] if self.segm is not None else None
        H.eval_facts([t["size"] for t in targets], self.facts, self.image_ids, origs=origs, ids=ids, mask_hw=hw)

    def _raw_facts(self, img, targets, host_ids):
        origs = [(int(im.shape[0]), int(im.shape[1])) for im in img.images]
        with_ids = "image_id" in targets[0]
        masks = self.canvas._masks(targets, True) if self.orig is not None else None
        H.eval_raw_facts(img.out_sizes(), origs, (self.canvas.height, self.canvas.width), self.facts, self.image_ids,
                         ids=host_ids if with_ids else None, mask_list=masks,
                         mask_table=self.orig.mask_table if masks is not None else None, max_pixels=self.max_pixels)
        if with_ids and host_ids is None:                    # ids that are on the device already are gathered there
            torch.stack([t["image_id"].reshape(()) for t in targets], out=self.image_ids)
        self._keep = masks                                   # the graph reads them through the table: alive until the next call

    def _tail(self, outputs):
        boxes = outputs["pred_boxes"]
        B, P, K, _ = boxes.shape
        pm = None
        if self.segm is not None:
            pm = outputs["pred_masks"]
            pm = (pm.squeeze(2) if pm.dim() == 5 else pm).to(torch.float32).contiguous()
        st = self.staged
        last = H.eval_canvas(boxes.to(torch.float32).contiguous(), outputs["phrase_mask"].reshape(B, P, K).to(torch.uint8).contiguous(),
                             st.targets_static[0], st.targets_static[1], self.facts, self.image_ids, self.state, pred_masks=pm,
                             tgt_masks=st.tgt_masks if pm is not None else None,
                             threshold=self.segm.threshold if self.segm is not None else 0.5, veto=self.fail_word)
        if self.orig is not None:
            H.eval_orig(pm, self.facts, self.orig, (self.canvas.height, self.canvas.width), threshold=self.segm.threshold,
                        veto=self.fail_word)
        return last

    @torch.no_grad()
    def __call__(self, samples, targets, host_ids=None):
        """Stages the batch, replays, and returns the loss meters' (names, device vector) -- a static buffer the next replay rewrites."""
        _before_forward_replay(self.inner)
        self.canvas.stage(samples, targets, out=self.staged, tokens=False)
        self._gather_facts(samples, targets, host_ids)
        _copy_batch(self.s, [], {k: v for k, v in samples.items() if k != "img"}, [])
        self.graph.replay()
        return self.names, self.vec


class _EvalPlan:
    """What decides how evaluate() runs its batches, read ONCE: the two environment switches, the device type, whether the
    post-processors are this package's (the meter reads PostProcessSegm's frame) and whether the criterion reads staged targets.
    replayed: the forward from a hipGraph per input shape; metered: scored on the device; on_canvas: through `canvas` -- refused before
    anything is launched where that cannot be done, ignored (said once) where the loop it would replace is off or not this package's."""

    def __init__(self, model, criterion, postprocessors, device, visualize, canvas, raw=False):
        """raw (evaluate_raw): a raw batch has nowhere else to go, so what would make `canvas` be ignored is refused instead."""
        from .models.post_process import PostProcessSegm, PostProcessVGMultiPhrase
        graph, metrics = (os.environ.get(k, "1") == "1" for k in ("REFTR_EVAL_GRAPH", "REFTR_EVAL_METRICS"))
        cuda = torch.device(device).type == "cuda"
        own_post = (isinstance(postprocessors["bbox"], PostProcessVGMultiPhrase)
                    and isinstance(postprocessors.get("segm", PostProcessSegm()), PostProcessSegm))
        self.replayed, self.metered, self.on_canvas = graph and cuda, metrics and cuda and own_post, False
        if canvas is None:
            return
        if _multi_rank():
            raise NotImplementedError("evaluate(canvas=) is not available on more than one rank: the box count the criterion normalises "
                                      "by is averaged over the ranks, and the count a canvas batch stages is this rank's")
        if visualize:
            raise NotImplementedError("evaluate(canvas=, visualize=True): the dumps need per-image masks_origin views, which a canvas "
                                      "evaluation never materialises")
        reasons = (("REFTR_EVAL_GRAPH=0", not graph), ("REFTR_EVAL_METRICS=0", not metrics), ("a CPU device", not cuda),
                   ("a post-processor that is not this package's", not own_post),
                   ("a criterion without targets_static", not hasattr(criterion, "targets_static")))
        why = next((text for text, holds in reasons if holds), None)               # the first that holds, in this order
        if why is not None and raw:
            raise NotImplementedError(f"evaluate_raw is not available with {why}: a raw batch is staged into the canvas's buffers and "
                                      "scored inside the captured graph, there is no other path for it")
        if why is not None:
            _say_once(model, ("eval-canvas", why), f"[reftr_amd] evaluate: {canvas!r} is ignored ({why}); every batch runs at its own shape")
        self.on_canvas = why is None


def _vis_dirs(output_dir, split):
    """output_dir/vis/<split>/{mask,bbox,att,gt} (engine_vg.py:86-94)."""
    from pathlib import Path
    if output_dir is None:
        raise ValueError("evaluate(visualize=True) needs an output_dir")
    root = Path(output_dir) / "vis" / str(split)
    for sub in ("mask", "bbox", "att", "gt"):
        (root / sub).mkdir(parents=True, exist_ok=True)
    return root


_VIS_PURPLE = (128, 0, 128)
_VIS_YELLOW = (255, 255, 0)


def _dump_visuals(root, dataset, dataset_id, mask_origin, pred_box, mask_att):
    """The four image dumps of one evaluated sample (engine_vg.py:157-192): `mask_origin` uint8 / bool [H, W] at the original
    image size (PostProcessSegm's 'masks_origin'), `pred_box` xyxy in original pixels, `mask_att` [heads, h, w] (the
    segmentation head's attention maps).  Host-side, off the hot path; PIL / matplotlib are imported here only."""
    import numpy as np
    from PIL import Image, ImageDraw
    import matplotlib
    matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    img, mask, _phrase, tgt_box, img_file = dataset.pull_item(dataset_id)
    pm = (mask_origin.detach().cpu().numpy() != 0)
    mask = np.asarray(mask)
    assert pm.shape == mask.shape[:2], (pm.shape, mask.shape)
    stem = str(img_file).split("/")[-1].split(".")[0]
    tag = f"{stem}_{dataset_id:05d}"
    purple = np.array(_VIS_PURPLE, dtype=np.uint8); yellow = np.array(_VIS_YELLOW, dtype=np.uint8)
    Image.fromarray(np.where(pm[..., None], yellow, purple)).save(root / "mask" / f"{tag}.jpg")
    Image.fromarray(np.where((mask != 0)[..., None], yellow, purple)).save(root / "gt" / f"{tag}.jpg")
    canvas = Image.fromarray(np.asarray(img))
    draw = ImageDraw.Draw(canvas)
    draw.rectangle([float(v) for v in pred_box.detach().cpu().reshape(-1)], outline="blue", width=5)
    draw.rectangle([float(v) for v in np.asarray(tgt_box).reshape(-1)], outline="red", width=5)
    canvas.save(root / "bbox" / f"{tag}.jpg")
    # attention maps: resized to 320 x 320 and cropped to the image's half size, heads 0, 1, 2 and 7 (:181-186)
    att = torch.nn.functional.interpolate(mask_att.detach().float().cpu()[None], size=(320, 320), mode="bilinear")[0].numpy()
    h, w = mask.shape[:2]
    for head in (0, 1, 2, 7):
        if head < att.shape[0]:
            plt.imsave(root / "att" / f"{tag}_{head}.jpg", att[head, :h // 2, :w // 2], cmap="viridis")


def _fill_results(results_dict, targets, results_scaled):
    """results_dict[image_id] = the image's scaled boxes as nested lists, from ONE device-to-host copy per batch for boxes and
    image ids together (float64 holds an fp32 box coordinate and an image id below 2^53 exactly)."""
    sel = [i for i, tg in enumerate(targets) if "image_id" in tg]
    if not sel:
        return
    dev = results_scaled[0]["boxes"].device
    ids = [targets[i]["image_id"] for i in sel]
    on_dev = [torch.is_tensor(v) and v.device == dev for v in ids]
    parts = [results_scaled[i]["boxes"].reshape(-1).double() for i in sel]
    if all(on_dev):
        parts.append(torch.stack([v.reshape(()) for v in ids]).double())
    flat = torch.cat(parts).cpu().tolist()
    if all(on_dev):
        ids = [int(v) for v in flat[len(flat) - len(sel):]]
    o = 0
    for i, image_id in zip(sel, ids):
        n = results_scaled[i]["boxes"].shape[0]
        results_dict[int(image_id)] = [flat[o + 4 * r: o + 4 * r + 4] for r in range(n)]
        o += 4 * n


def _stacked_sizes(targets, original=False):
    """[B, 2] (h, w) of the batch's images as the model saw them, or (`original`) before resizing where the targets say."""
    key = "orig_size" if original and "orig_size" in targets[0] else "size"
    return torch.stack([t[key] for t in targets], dim=0)


class _LoaderOrder:
    """The way every batch's results reach results_dict, in loader order: per batch one (book, index), `book` a list of dicts --
    `filled`, filled batch by batch (fill()), or a results ring's slots, empty until the ring is read back and decoded (slot())."""

    def __init__(self):
        self.order, self.filled = [], []

    def fill(self):
        self.filled.append({})
        self.slot(self.filled, len(self.filled) - 1)
        return self.filled[-1]

    def slot(self, book, index):
        self.order.append((book, index))

    def merge(self, results_dict):
        for book, index in self.order:
            results_dict.update(book[index])


class _OwnShapeEval:
    """A batch evaluated at its own shape: the forward (`replayed`: CapturedForward, else the model's launches), run again on the
    launched chain when a hand-off timed out; criterion; the loss meters, handed to `book(names, vec)` BEFORE the subclass's score():
    scoring waits for the device, and what is launched before it costs the host nothing.  vis: None or (directory, dataset)."""

    def __init__(self, model, criterion, postprocessors, device, replayed, vis, book):
        fwd = CapturedForward(model) if replayed else model
        self.losses = _ForwardLosses(lambda samples: _run_again_on_chain(model, lambda: fwd(samples)), criterion)
        self.post, self.device, self.vis, self.book, self.order = postprocessors, device, vis, book, _LoaderOrder()

    def __call__(self, batch_no, samples, targets):
        outputs, names, vec = self.losses(samples, targets)
        self.book(names, vec)
        self.score(outputs, targets, _stacked_sizes(targets, original=True))
        return outputs

    def dump_visuals(self, outputs, targets, results, results_scaled):
        if self.vis is not None:
            for res, tg, scaled, att in zip(results, targets, results_scaled, outputs["mask_att"]):
                _dump_visuals(*self.vis, int(tg["dataset_id"]), res["masks_origin"][0, 0], scaled["boxes"][0], att)


class _TorchLoopEval(_OwnShapeEval):
    """The reference's per-image torch loop (engine_vg.py:127-152, 205-219): Acc@0.5 and mean IoU of the predicted boxes, mean mask
    IoU with a 'segm' post-processor; the running sums stay on the device until finish()."""

    def __init__(self, *args):
        super().__init__(*args)
        self.sum_accu, self.sum_iou, self.cnt, self.seg_iou = (torch.zeros((), device=self.device) for _ in range(4))
        self.cnt_seg = 0.0

    def score(self, outputs, targets, orig_sizes):
        results = self.post["bbox"](outputs, orig_sizes)
        for res, tg in zip(results, targets):
            gt = box_cxcywh_to_xyxy(tg["boxes"])
            assert gt.size(0) == res["boxes"].size(0), (res, gt)
            iou = torch.diag(box_iou(gt, res["boxes"])[0])
            self.sum_accu += (iou > 0.5).float().sum(); self.sum_iou += iou.sum(); self.cnt += len(tg["boxes"])
        results_scaled = self.post["bbox"](outputs, orig_sizes, scale_to_original_shape=True)
        if "segm" in self.post:
            results = self.post["segm"](results, outputs, orig_sizes, _stacked_sizes(targets))
            for res, tg in zip(results, targets):
                self.seg_iou += mask_iou(res["masks"][0][0], tg["masks"])
                self.cnt_seg += 1
            self.dump_visuals(outputs, targets, results, results_scaled)
        filled = self.order.fill()
        for tg, res in zip(targets, results_scaled):             # the reference's fill, one copy per image (:203)
            if "image_id" in tg:
                filled[int(tg["image_id"])] = res["boxes"].cpu().numpy().tolist()

    def finish(self, stats, results_dict):
        if utils.is_dist_avail_and_initialized():
            for t in (self.sum_accu, self.sum_iou, self.cnt) + ((self.seg_iou,) if "segm" in self.post else ()):
                torch.distributed.all_reduce(t)
        stats["accuracy_iou0.5"] = float(self.sum_accu / self.cnt.clamp(min=1))
        stats["miou"] = float(self.sum_iou / self.cnt.clamp(min=1))
        if "segm" in self.post:                  # the reference's formula: sum / (world x this rank's sample count), :212-219
            stats["seg_miou"] = float(self.seg_iou / max(utils.get_world_size() * self.cnt_seg, 1.0))
        self.order.merge(results_dict)


class _MeteredEval(_OwnShapeEval):
    """Scored on the device by metrics.EvalMeter (csrc/rt_eval.hip: one ABI call per batch, the running totals are read back once),
    which adds 'seg_oiou' and 'seg_prec@0.5' ... '@0.9' for a RES model.  One device-to-host copy per batch: the result boxes."""

    def __init__(self, *args):
        super().__init__(*args)
        self.meter = EvalMeter(self.device, seg="segm" in self.post)

    def score(self, outputs, targets, orig_sizes):
        results_scaled = self.post["bbox"](outputs, orig_sizes, scale_to_original_shape=True)
        for res, tg in zip(results_scaled, targets):         # the reference's check, on the post-processor's host counts
            assert tg["boxes"].size(0) == res["boxes"].size(0), (res, tg["boxes"])
        if "segm" in self.post:
            frame = self.post["segm"].frame(outputs, orig_sizes, _stacked_sizes(targets))
            self.meter.update(outputs, targets, masks=frame[0], sizes=frame[2])
            if self.vis is not None:                         # the dumps alone need per-image views
                self.dump_visuals(outputs, targets, self.post["segm"].views([{} for _ in targets], frame), results_scaled)
        else:
            self.meter.update(outputs, targets)
        _fill_results(self.order.fill(), targets, results_scaled)

    def finish(self, stats, results_dict):
        stats.update(self.meter.compute())
        self.order.merge(results_dict)


class _CanvasEval:
    """A batch that fits `canvas` (why_not, why_not_eval) runs as one replay of one captured graph (CapturedEvalStep; one capture per
    canvas key) with no device-to-host copy: totals and boxes stay on the device, in the wrapped _MeteredEval's accumulators and a results
    ring per key, read back once in finish().  A batch that does not fit goes to that path at its own shape (said once per reason).  A
    replay whose hand-off timed out was vetoed on the device: every capture goes, the rings stay, the batch is replayed once more.

    The fit test follows the form of the batch.  A RAW batch (evaluate_raw) is asked why_not and why_not_eval_raw; one that does not fit
    is converted once by the existing device chain (BatchCanvas.resized_eval) and goes to the same own-shape path, and with a 'segm'
    post-processor its original-frame mask totals are added by the same two ABI calls, eagerly (_orig_own_shape).  `host_ids`: the
    coming raw batch's image ids as python ints where the loader delivered them in host memory (set by evaluate_raw per batch)."""

    def __init__(self, model, criterion, postprocessors, canvas, slots, own_shape):
        assert isinstance(own_shape, _MeteredEval)           # its meter, loader order and `book` are this path's too
        self.model, self.canvas, self.slots, self.capture_args = model, canvas, slots, (model, criterion, postprocessors, canvas)
        self.own_shape, self.meter, self.order, self.segm = own_shape, own_shape.meter, own_shape.order, "segm" in postprocessors
        self.steps, self.rings = {}, {}      # by canvas key: the capture; (the ring's device state, its batches as replayed, decoded)
        self.post, self.host_ids, self._keep_orig = postprocessors, None, None
        self.meter.reset(fresh=False)

    def _replay(self, key, samples, targets):
        step = self.steps.get(key)
        if step is None:
            state = self.rings[key][0] if key in self.rings else None
            step = self.steps[key] = CapturedEvalStep(*self.capture_args, samples, targets, self.meter.acc, self.slots, state=state,
                                                      acc_orig=self.meter.acc_orig, host_ids=self.host_ids)
            self.rings.setdefault(key, (step.state, [], []))
        return step(samples, targets, self.host_ids) if step.raw else step(samples, targets)

    def _orig_own_shape(self, outputs, frame_hw, samples, targets):
        """The original-frame mask totals of a raw batch that ran at its own shape: rt_eval_raw_facts + rt_eval_orig, eagerly, with
        the batch's own padded size as the frame and its largest image as max_pixels.  An image whose target mask does not have its
        size cannot be scored on its frame: its table entry is zeroed and it contributes nothing."""
        pm = outputs["pred_masks"]
        pm = (pm.squeeze(2) if pm.dim() == 5 else pm).to(torch.float32).contiguous()
        img, n, keep = samples["img"], H.BATCH_STAGE_MAX_B, []
        for b0 in range(0, len(img), n):                     # (a batch of more than RT_BATCH_STAGE_MAX_B images: in slices)
            ims, sizes, tg = img.images[b0:b0 + n], img.out_sizes()[b0:b0 + n], targets[b0:b0 + n]
            origs = [(int(im.shape[0]), int(im.shape[1])) for im in ims]
            tm = [t.get("masks") for t in tg]
            ok = [m is not None and m.dim() == 3 and m.shape[0] == 1 and tuple(m.shape[-2:]) == o for m, o in zip(tm, origs)]
            masks = [(m if m.element_size() == 1 else m.float() > 0.5).contiguous() if k
                     else torch.zeros(o, dtype=torch.uint8, device=pm.device) for m, o, k in zip(tm, origs, ok)]
            st = H.EvalOrigState(len(ims), max(h * w for h, w in origs), pm.device, acc=self.meter.acc_orig)
            facts = torch.zeros((len(ims), 6), dtype=torch.int32, device=pm.device)
            H.eval_raw_facts(sizes, origs, frame_hw, facts, torch.zeros(len(ims), dtype=torch.int64, device=pm.device), mask_list=masks,
                             mask_table=st.mask_table, max_pixels=st.max_pixels)
            if not all(ok):
                st.mask_table.mul_(torch.tensor([int(k) for k in ok], dtype=torch.int64).to(pm.device, non_blocking=True))
            H.eval_orig(pm[b0:b0 + n].contiguous(), facts, st, frame_hw, threshold=self.post["segm"].threshold)
            keep.append((st, facts, masks))
        self._keep_orig = (keep, pm)                         # alive until the next such batch

    def __call__(self, batch_no, samples, targets):
        raw = _is_raw(samples)
        why = self.canvas.why_not(samples, targets) or (self.canvas.why_not_eval_raw(samples, targets, segm=self.segm) if raw else
                                                        self.canvas.why_not_eval(samples, targets, segm=self.segm))
        if why is not None and raw:
            _say_once(self.model, ("eval-canvas", why), f"[reftr_amd] evaluate_raw: a raw batch does not fit {self.canvas!r} ({why}): "
                      "it is resized by the DeviceInputPipeline chain and runs at its own shape")
            ns, nt = self.canvas.resized_eval(samples, targets)
            outputs = self.own_shape(batch_no, ns, nt)
            if self.segm:
                self._orig_own_shape(outputs, tuple(ns["img"].tensors.shape[-2:]), samples, targets)
            return None
        if why is not None:
            _say_once(self.model, ("eval-canvas", why), f"[reftr_amd] evaluate: a batch does not fit {self.canvas!r} ({why}): it runs at "
                      "its own shape")
            return self.own_shape(batch_no, samples, targets)
        key = self.canvas.key(samples)
        if any(st._gen != _state(self.model).coop_generation for st in self.steps.values()):
            self.steps.clear()
        self.own_shape.book(*_run_again_on_chain(self.model, lambda: self._replay(key, samples, targets), drop=self.steps.clear))
        self.meter.book(len(targets), self.segm)
        _, batches, decoded = self.rings[key]
        self.order.slot(decoded, len(batches))
        batches.append((batch_no, "image_id" in targets[0], [int(t["boxes"].shape[0]) for t in targets]))

    def finish(self, stats, results_dict):
        for st, batches, decoded in self.rings.values():         # the ONE read-back of the result boxes, then a pure host decode
            decoded += decode_ring(st.boxes.cpu().numpy(), st.counts.cpu().numpy(), st.ids.cpu().numpy(), *st.cursor.tolist(), batches)
        self.own_shape.finish(stats, results_dict)


@torch.no_grad()
def evaluate(model, criterion, postprocessors, data_loader, device, output_dir=None, visualize=False, canvas=None):
    """engine_vg.evaluate (engine_vg.py:82-225): the loss meters, Acc@0.5 / mean IoU of the predicted boxes, mask IoU with a 'segm'
    post-processor, and the boxes scaled to the original image size in the returned results dict (:141,203).  How a batch is evaluated
    is chosen once (_EvalPlan): scored on the device (_MeteredEval) or by the reference's torch loop (_TorchLoopEval), and with `canvas`
    (a reftr_amd.data.canvas.BatchCanvas, which defines what a canvas batch computes) replayed from one graph where it fits (_CanvasEval).
    `visualize` (needs 'segm', `output_dir` and a dataset with `split` / `pull_item`): _dump_visuals' images per sample (:86-96,157-192).
    A path books a batch's loss meters on the board itself (board.add_device, handed to it), before whatever waits for the device."""
    plan = _EvalPlan(model, criterion, postprocessors, device, visualize, canvas)
    model.eval()
    criterion.eval()
    board = utils.StatBoard()
    vis = (_vis_dirs(output_dir, data_loader.dataset.split), data_loader.dataset) if visualize else None
    own_shape = _MeteredEval if plan.metered else _TorchLoopEval
    path = own_shape(model, criterion, postprocessors, device, plan.replayed, vis, board.add_device)
    if plan.on_canvas:
        path = _CanvasEval(model, criterion, postprocessors, canvas, len(data_loader), path)
    prefetcher = data_prefetcher(data_loader, device, prefetch=True)
    samples, targets = prefetcher.next()
    for batch_no in board.log_every(range(len(data_loader)), 50, "Test:"):
        if _is_raw(samples):
            raise NotImplementedError("evaluate: a raw batch (reftr_amd.data.RawImages) is not taken: the metric tail reads the resized "
                                      "`size` of every image from device memory (rt_eval_facts), which a raw batch has on the host only; "
                                      "evaluate_raw takes it")
        path(batch_no, samples, targets)
        samples, targets = prefetcher.next()
    _check_cooperative(model)
    board.synchronize_between_processes()
    stats, results_dict = board.global_avg(), {}
    path.finish(stats, results_dict)
    return {k: v for k, v in stats.items() if k.split("_")[-1] not in ("unscaled", "0", "1", "2")}, results_dict      # engine_vg.py:221


@torch.no_grad()
def evaluate_raw(model, criterion, postprocessors, data_loader, device, canvas, output_dir=None):
    """evaluate() for a loader of RAW batches (reftr_amd.data.raw: samples["img"] a RawImages on the host or the device, targets in the
    raw frame -- `boxes` xyxy pixels, with a 'segm' post-processor a one-byte [1, h, w] `masks` of the image's own size, `image_id` one
    int64 on all targets or on none; `size` and `orig_size` are not read, they are RawImages.out_sizes() and the raw (h, w)).
    -> (stats, results_dict).

    The existing keys and results_dict are what evaluate(canvas=canvas) returns on the batches converted by BatchCanvas.resized_eval
    (the DeviceInputPipeline chain, `size` / `orig_size` / `image_id` as tensors).  With a 'segm' post-processor the stats also carry
    'seg_miou_orig', 'seg_oiou_orig' and 'seg_prec@0.5_orig' ... '@0.9_orig': metrics.stats_from_orig_accumulators over integer {I, U}
    counted on the raw h x w frame, query 0's masks_origin (Predictor's mask: the canvas as the frame) against the raw mask bytes.
    Per fitting batch the host issues rt_raw_stage, rt_eval_raw_facts, the grouped token copy and ONE replay of the one graph per
    canvas key; a batch that does not fit (why_not, why_not_eval_raw) is converted once and runs at its own shape, said once per
    reason, adding to the same totals.  Refused before anything is launched: more than one rank, the data-parallel wrapper, a CPU
    device, foreign post-processors, a criterion without targets_static, REFTR_EVAL_GRAPH=0 / REFTR_EVAL_METRICS=0 (a raw batch has
    nowhere else to go); a batch that is not raw raises TypeError.  The model's and the criterion's train / eval mode and the
    criterion's targets_static are restored on exit."""
    import itertools
    if canvas is None:
        raise NotImplementedError("evaluate_raw needs a canvas: rt_raw_stage writes a raw batch into a canvas's buffers")
    _canvas_single_process(model)
    plan = _EvalPlan(model, criterion, postprocessors, device, False, canvas, raw=True)
    assert plan.on_canvas and plan.metered
    loader = iter(data_loader)
    first = next(loader, None)
    if first is not None and not _is_raw(first[0]):          # (before anything touches the device)
        raise TypeError("evaluate_raw takes raw batches: samples['img'] must be a reftr_amd.data.RawImages, not "
                        f"{type(first[0].get('img') if isinstance(first[0], dict) else first[0]).__name__}")
    if first is not None:
        _no_gains(first[0], 0)
    modes =(model.training, criterion.training)
    static = (criterion.targets_static, getattr(criterion, "target_masks_static", None))
    model.eval()
    criterion.eval()
    try:
        criterion.targets_static = None                      # (a batch at its own shape reads its targets from the list)
        if hasattr(criterion, "target_masks_static"):
            criterion.target_masks_static = None
        board = utils.StatBoard()
        own_shape = _MeteredEval(model, criterion, postprocessors, device, plan.replayed, None, board.add_device)
        path = _CanvasEval(model, criterion, postprocessors, canvas, len(data_loader), own_shape)
        if "segm" in postprocessors:
            path.meter.book_orig()
        batches = itertools.chain([first] if first is not None else [], loader)
        for batch_no in board.log_every(range(len(data_loader)), 50, "Test:"):
            samples, targets = next(batches)
            if not _is_raw(samples):
                raise TypeError(f"evaluate_raw takes raw batches: batch {batch_no} has no reftr_amd.data.RawImages")
            _no_gains(samples, batch_no)
            ids = [t.get("image_id") for t in targets]
            # ids the loader left in host memory travel by value (free to read here); ids on the device are gathered there
            path.host_ids = ([int(v) for v in ids] if ids and all(torch.is_tensor(v) and not v.is_cuda and v.numel() == 1 for v in ids)
                             else None)
            if not _on_device(samples):                      # a host batch: the raw bytes cross, everything else happens on the device
                samples, targets = _to_device(samples, targets, device)
            path(batch_no, samples, targets)
        _check_cooperative(model)
        board.synchronize_between_processes()
        stats, results_dict = board.global_avg(), {}
        path.finish(stats, results_dict)
    finally:
        model.train(modes[0])
        criterion.train(modes[1])
        criterion.targets_static = static[0]
        if hasattr(criterion, "target_masks_static"):
            criterion.target_masks_static = static[1]
    return {k: v for k, v in stats.items() if k.split("_")[-1] not in ("unscaled", "0", "1", "2")}, results_dict
