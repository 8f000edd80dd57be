#!/usr/bin/env python3
"""Prediction-error timing probe (include/fme_merge.h).

One 1080p frame's PUs (synth.make_ctu_jobs, one entry per PU), five merge candidates plus the ME
motion each, as one fme_pred_error_device batch: the k_pred_err time from fme_pred_error_last_ms
(median of 20 launches after 3 warm-ups) and the tasks per second, at 8 and 10 bits; then the
one-core rate of the reference composition the fixtures use (oracle/_ref: Reference.mc + Reference.satd
per task) on a 20,000-task sample of the same list, where that library is built.  Prints one JSON
line per measurement.  No figure is compared against a target.

The VALU figure is a static count of the kernel's arithmetic per 4x4 unit (lane-ops): per predicted
list 11 window rows x (3 re-alignments + 4 columns x (2 byte funnels + 2 dot4)) = 209 (at 10 bits,
without dot4: 121 sample offsets + 11 x 4 x 8 multiply-adds + 44 shifts = 517), the vertical
stage 16 x 8 multiply-adds + 16 x 4 rounding / clipping = 192; bi-prediction adds 16 x 4 for addAvg;
the distortion 16 subtractions + 64 butterfly adds + 32 for the absolute sums = 112, with 8x8
Hadamards 64 more (32 cross-lane moves, 32 adds).  Roof: 256 CUs x 4 SIMDs x 32 lanes/clk x 2.4 GHz.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd"), os.path.join(ROOT, "oracle")]

W, H = 1920, 1080
VALU_ROOF = 256 * 4 * 32 * 2.4e9   # lane-ops/s


def frame_tasks(rng):
    from nnfme import merge, synth
    pus = synth.make_ctu_jobs(rng, W, H, 423, 0, [1], [0])
    n = len(pus)
    t = np.zeros((n, 6), merge.PE_TASK_DTYPE)
    cu = np.array([merge.cu_origin(*v) for v in zip(pus["x"], pus["y"], pus["w"], pus["h"])])
    for f in ("x", "y", "w", "h"):
        t[f] = pus[f][:, None]
    t["cu_x"], t["cu_y"] = cu[:, 0:1], cu[:, 1:2]
    t["org_id"] = 0
    t["flags"] = rng.choice([1, 2, 3], size=(n, 6), p=[0.45, 0.2, 0.35])
    t["ref_id"] = rng.integers(1, 4, (n, 6, 2))
    near = 4 * np.stack([pus["mv_x"], pus["mv_y"]], axis=-1).astype(np.int64)   # the PU's own motion
    t["mv"] = np.clip(near[:, None, None, :] + rng.integers(-12, 13, (n, 6, 2, 2)), -32768, 32767)
    return t.reshape(-1)


def lane_ops(tasks, bit_depth=8):
    units = (tasks["w"].astype(np.int64) // 4) * (tasks["h"] // 4)
    bi = (tasks["flags"] & 3) == 3
    same = bi & (tasks["ref_id"][:, 0] == tasks["ref_id"][:, 1]) & (tasks["mv"][:, 0] == tasks["mv"][:, 1]).all(axis=1)
    lists = np.where(bi & ~same, 2, 1)
    had8 = ((tasks["w"] | tasks["h"]) & 7) == 0
    first = 209 if bit_depth == 8 else 121 + 352 + 44
    per_unit = lists * (first + 192) + np.where(lists == 2, 64, 0) + 112 + np.where(had8, 64, 0)
    return int((units * per_unit).sum())


def gpu_rate(tasks, bit_depth):
    import torch
    from nnfme import merge, synth
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=0, use_hadamard=1, bit_depth=bit_depth)
    try:
        for k in range(4):
            ctx.set_picture(k, synth.synth_luma(W, H, k) if bit_depth == 8 else synth.synth_luma_hbd(W, H, k, bit_depth))
        d_tasks = torch.from_numpy(tasks.view(np.uint8).copy()).cuda()
        d_dist = torch.zeros(len(tasks), dtype=torch.int32, device="cuda")
        ctx.set_profiling(True)
        ms = []
        for i in range(23):
            merge.pred_error_device(ctx, d_tasks, d_dist, len(tasks))
            ms.append(merge.pred_error_last_ms(ctx))
        assert merge.pred_error_invalid_count(ctx) == 0
        med = float(np.median(ms[3:]))
        ops = lane_ops(tasks, bit_depth)
        print(json.dumps({"probe": "k_pred_err", "bit_depth": bit_depth, "tasks": len(tasks), "ms_median": round(med, 4),
                          "ms_min": round(min(ms[3:]), 4), "ms_max": round(max(ms[3:]), 4),
                          "tasks_per_s": round(len(tasks) / (med * 1e-3)), "lane_ops": ops,
                          "valu_roof_fraction": round(ops / (med * 1e-3) / VALU_ROOF, 4)}), flush=True)
        return d_dist.cpu().numpy().view(np.uint32)
    finally:
        ctx.close()


def ref_rate(tasks, got, sample=20000):
    from nnfme import synth
    from nnfme.abi import MC_JOB_DTYPE
    from oracle import REF_SO, Reference
    if not os.path.exists(REF_SO):
        print(json.dumps({"probe": "ref_composition", "skipped": "oracle/_ref is not built"}), flush=True)
        return
    ref = Reference(use_hadamard=1)
    luma = [synth.synth_luma(W, H, k) for k in range(4)]
    flat = np.full((H // 2, W // 2), 128, np.uint8)
    for k in range(4):
        ref.set_picture_yuv(k, luma[k], flat, flat)
    idx = np.random.default_rng(3).choice(len(tasks), sample, replace=False)
    jobs = np.zeros(sample, MC_JOB_DTYPE)
    for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv"):
        jobs[f] = tasks[f][idx]
    jobs["flags"] = tasks["flags"][idx] & 3
    y, cb, cr = np.zeros((H, W), np.uint8), flat.copy(), flat.copy()
    out = np.zeros(sample, np.uint32)
    t0 = time.perf_counter()
    for i in range(sample):
        ref.mc(jobs[i:i + 1], y, cb, cr)
        j = jobs[i]
        x0, y0, w, h = int(j["x"]), int(j["y"]), int(j["w"]), int(j["h"])
        out[i] = ref.satd(luma[0][y0:y0 + h, x0:x0 + w], y[y0:y0 + h, x0:x0 + w], True)
    dt = time.perf_counter() - t0
    print(json.dumps({"probe": "ref_composition", "tasks": sample, "seconds": round(dt, 3),
                      "tasks_per_s": round(sample / dt), "equal_to_gpu": bool(np.array_equal(out, got[idx]))}), flush=True)


def main():
    tasks = frame_tasks(np.random.default_rng(7))
    got8 = gpu_rate(tasks, 8)
    gpu_rate(tasks, 10)
    ref_rate(tasks, got8)


if __name__ == "__main__":
    main()
