"""CPU: the host side of the device evaluation metrics (reftr_amd/metrics.py) -- the statistics from the accumulator slots, the
per-image table built from tensor shapes, and the all-reduce of the slots over a gloo world of 2."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from reftr_amd import hip as H
from reftr_amd import metrics as M

NEW_KEYS = {"seg_oiou", "seg_prec@0.5", "seg_prec@0.6", "seg_prec@0.7", "seg_prec@0.8", "seg_prec@0.9"}


def _slots(det_n=0, det_hit=(0,) * 5, seg_n=0, seg_hit=(0,) * 5, seg_i=0, seg_u=0, det_sum=0.0, seg_sum=0.0):
    s = [0] * H.EVAL_SLOTS
    s[H.EVAL_DET_N] = det_n; s[H.EVAL_SEG_N] = seg_n; s[H.EVAL_SEG_I] = seg_i; s[H.EVAL_SEG_U] = seg_u
    s[H.EVAL_DET_HIT:H.EVAL_DET_HIT + 5] = det_hit; s[H.EVAL_SEG_HIT:H.EVAL_SEG_HIT + 5] = seg_hit
    s[H.EVAL_DET_SUM] = det_sum; s[H.EVAL_SEG_SUM] = seg_sum
    return s


def test_slot_indices_match_the_header():
    """The binding's slot indices and chunk size are the header's enum / macro values."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "reftr_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"RT_EVAL_([A-Z_]+) = (\d+)", src))
    assert enum == {"DET_N": H.EVAL_DET_N, "DET_HIT": H.EVAL_DET_HIT, "SEG_N": H.EVAL_SEG_N, "SEG_HIT": H.EVAL_SEG_HIT,
                    "SEG_I": H.EVAL_SEG_I, "SEG_U": H.EVAL_SEG_U, "DET_SUM": H.EVAL_DET_SUM, "SEG_SUM": H.EVAL_SEG_SUM,
                    "SLOTS": H.EVAL_SLOTS}
    assert int(re.search(r"#define RT_EVAL_CHUNK (\d+)", src).group(1)) == H.EVAL_CHUNK
    assert H.EVAL_SLOTS == 16 and H.EVAL_DET_HIT + 5 == H.EVAL_SEG_N and H.EVAL_SEG_HIT + 5 == H.EVAL_SEG_I


def test_stats_from_accumulators_hand_filled():
    s = _slots(det_n=7, det_hit=(3, 2, 2, 1, 0), det_sum=3.25, seg_n=4, seg_hit=(4, 3, 2, 1, 0), seg_i=300, seg_u=1200, seg_sum=2.5)
    rec = M.stats_from_accumulators(s)
    assert set(rec) == {"accuracy_iou0.5", "miou"}                               # no mask key without a segm post-processor
    assert rec["accuracy_iou0.5"] == float(np.float32(3) / np.float32(7))        # the fp32 quotient evaluate() always reported
    assert rec["miou"] == 3.25 / 7
    res = M.stats_from_accumulators(s, seg=True, world=1, local_seg_n=4)
    assert set(res) == {"accuracy_iou0.5", "miou", "seg_miou"} | NEW_KEYS
    assert res["seg_miou"] == 2.5 / 4 and res["seg_oiou"] == 0.25
    assert [res[f"seg_prec@{t}"] for t in M.THRESHOLDS] == [1.0, 0.75, 0.5, 0.25, 0.0]
    # the reference divides the all-reduced sum by world x THIS rank's sample count (engine_vg.py:212-219), whatever the others had:
    # summed slots of two ranks that scored 4 and 3 samples, seen from the rank that scored 3
    s2 = _slots(seg_n=7, seg_hit=(7, 0, 0, 0, 0), seg_i=10, seg_u=40, seg_sum=4.5)
    r2 = M.stats_from_accumulators(s2, seg=True, world=2, local_seg_n=3)
    assert r2["seg_miou"] == 4.5 / 6 and r2["seg_prec@0.5"] == 1.0 and r2["seg_prec@0.6"] == 0.0 and r2["seg_oiou"] == 0.25


def test_stats_from_accumulators_zero_counts_clamp():
    """Nothing scored: the counts clamp to 1 as the loop's cnt.clamp(min=1) / max(cnt_seg, 1.0) do; 0 / 0 pixels is NaN."""
    z = M.stats_from_accumulators(_slots(), seg=True, world=2, local_seg_n=0)
    assert z["accuracy_iou0.5"] == 0.0 and z["miou"] == 0.0 and z["seg_miou"] == 0.0
    assert all(z[f"seg_prec@{t}"] == 0.0 for t in M.THRESHOLDS) and math.isnan(z["seg_oiou"])
    n = M.stats_from_accumulators(_slots(det_n=2, det_sum=float("nan")))
    assert math.isnan(n["miou"]) and n["accuracy_iou0.5"] == 0.0


def _bytes_at(ptr, n):
    return bytes((ctypes.c_ubyte * n).from_address(ptr))


def test_table_builder_on_cpu_tensors():
    g = torch.Generator().manual_seed(5)
    wide = torch.rand(9, 26, generator=g) < 0.5
    targets = [
        {"boxes": torch.rand(2, 4, generator=g), "masks": torch.rand(7, 13, generator=g) < 0.5},                       # [h, w] bool
        {"boxes": torch.rand(0, 4, generator=g), "masks": (torch.rand(1, 5, 3, generator=g) < 0.5).to(torch.uint8)},   # [1, h, w] uint8
        {"boxes": torch.rand(6, 4, generator=g)[::2], "masks": wide[:, ::2]},                                          # both non-contiguous
        {"boxes": torch.rand(1, 4, generator=g), "masks": (torch.rand(1, 4, 4, generator=g) < 0.5)},                   # [1, h, w] bool
    ]
    sizes = [(7, 13), (5, 3), (9, 13), (4, 4)]
    words, keep = M.build_table(targets, sizes)
    B = len(targets)
    assert words.dtype == torch.int64 and words.device.type == "cpu" and words.numel() == 6 * B
    table = words[:5 * B].view(B, 5).tolist()
    assert words[5 * B:].view(torch.int32).view(B, 2).tolist() == [list(s) for s in sizes]      # the kernel's int32 [B, 2] view
    kept = {t.data_ptr(): t for t in keep}
    for b, (row, tg) in enumerate(zip(table, targets)):
        boxes, m = kept[row[0]], kept[row[2]]
        assert row[1] == tg["boxes"].shape[0] and (row[3], row[4]) == sizes[b]
        assert boxes.is_contiguous() and boxes.dtype == torch.float32 and torch.equal(boxes, tg["boxes"])
        assert m.is_contiguous() and m.element_size() == 1 and tuple(m.shape) == sizes[b]
        want = tg["masks"].reshape(sizes[b]) != 0
        assert torch.equal(m != 0, want)
        # what the kernel reads at that pointer: one byte per pixel at pitch = width
        raw = np.frombuffer(_bytes_at(row[2], m.numel()), dtype=np.uint8).reshape(sizes[b])
        assert np.array_equal(raw != 0, want.numpy())
        if boxes.numel():
            assert np.array_equal(np.frombuffer(_bytes_at(row[0], boxes.numel() * 4), dtype=np.float32).reshape(-1, 4), tg["boxes"].numpy())
    # contiguous inputs are named in place, not copied
    assert table[0][0] == targets[0]["boxes"].data_ptr() and table[0][2] == targets[0]["masks"].data_ptr()
    assert table[1][2] == targets[1]["masks"].data_ptr() and table[2][2] != wide.data_ptr()
    # boxes only: no mask pointer, no sizes words
    w2, _ = M.build_table(targets)
    assert w2.numel() == 5 * B and [r[2:] for r in w2.view(B, 5).tolist()] == [[0, 0, 0]] * B


def test_table_builder_rejects_a_target_of_another_size():
    """The reference's mask_iou asserts target.shape[-2:] == masks.shape[-2:]; the meter keeps it, on the host."""
    tg = [{"boxes": torch.zeros(1, 4), "masks": torch.zeros(1, 7, 13, dtype=torch.bool)}]
    M.build_table(tg, [(7, 13)])
    for bad in ((7, 12), (13, 7), (8, 13)):
        with pytest.raises(AssertionError):
            M.build_table(tg, [bad])


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _rank_slots(rank):
    if rank == 0:
        return _slots(det_n=5, det_hit=(4, 3, 2, 1, 0), det_sum=2.75, seg_n=4, seg_hit=(3, 3, 1, 1, 1), seg_i=1000, seg_u=3000, seg_sum=2.25)
    return _slots(det_n=3, det_hit=(1, 1, 1, 0, 0), det_sum=0.5 + 2.0 ** -30, seg_n=3, seg_hit=(1, 0, 0, 0, 0), seg_i=2 ** 40, seg_u=2 ** 41 + 1000,
                  seg_sum=1.125)


def _meter_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        meter = M.EvalMeter("cpu", seg=True)
        s = _rank_slots(rank)
        meter.acc[:H.EVAL_DET_SUM] = torch.tensor(s[:H.EVAL_DET_SUM], dtype=torch.int64)
        meter.acc[H.EVAL_DET_SUM:].view(torch.float64)[:] = torch.tensor(s[H.EVAL_DET_SUM:], dtype=torch.float64)
        meter.local_seg_n = s[H.EVAL_SEG_N]
        before = meter.acc.clone()
        local = meter.compute(world_reduce=False)
        summed = meter.compute()
        again = meter.compute()                                  # compute() leaves the accumulators as they were
        q.put((rank, local, summed, again == summed and torch.equal(meter.acc, before)))
    finally:
        dist.destroy_process_group()


def test_meter_compute_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_meter_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = _rank_slots(0), _rank_slots(1)
    tot = [x + y for x, y in zip(a, b)]                          # python ints: exact; the doubles are exactly representable sums
    for rank, local, summed, stable in res:
        mine = (a, b)[rank]
        assert stable
        assert local == M.stats_from_accumulators(mine, seg=True, world=1, local_seg_n=mine[H.EVAL_SEG_N])
        assert summed == M.stats_from_accumulators(tot, seg=True, world=2, local_seg_n=mine[H.EVAL_SEG_N])
        assert summed["accuracy_iou0.5"] == float(np.float32(5) / np.float32(8)) and summed["miou"] == (3.25 + 2.0 ** -30) / 8
        assert summed["seg_oiou"] == (1000 + 2 ** 40) / (4000 + 2 ** 41)          # int64 counts past 2^32 survive the reduce
        assert [summed[f"seg_prec@{t}"] for t in M.THRESHOLDS] == [4 / 7, 3 / 7, 1 / 7, 1 / 7, 1 / 7]
        assert summed["seg_miou"] == 3.375 / (2 * mine[H.EVAL_SEG_N])
