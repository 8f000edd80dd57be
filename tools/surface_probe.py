#!/usr/bin/env python3
"""Cost-surface timing probe (include/fme_surface.h).

One synthetic 1080p LDP frame's jobs (synth.make_ctu_jobs, 423 calls per CTU and reference, 4
references: 862,920 jobs) as one fme_cost_surface_device batch, at 8 and 10 bits: the
k_cost_surface time from fme_cost_surface_last_ms (device events around the launch).  The baseline
is the only way to get the same numbers without the kernel: fme_pred_error_device with 49 tasks
per job (one per quarter-pel position, FME_MC_L0 at the MV 4 mv + (dx, dy)) on the frame's uni-pred,
unkeyed jobs, timed by fme_pred_error_last_ms.  The two alternate in one process (3 warm-up rounds,
then 12 timed rounds of surface / baseline); medians, extremes, their ratio, and how many distortion
words of the two agree are printed as one JSON line per bit depth.  (The baseline applies clipMv
against the CTU origin, which the surface does not: words differ only where that clip bites.)  No
figure is compared against a target.

The VALU figure is a static count of the kernel's arithmetic per 4x4 unit (lane-ops).  At 8 bits:
the window's 12 x 3 re-alignments = 36; per dx 12 rows x 4 columns x (2 byte funnels + 2 dot4) = 192,
seven times; per position the vertical stage 16 x 8 multiply-adds + 16 x 4 rounding / clipping = 192,
the distortion 16 subtractions + 64 butterfly adds + 32 for the absolute sums = 112 (with 8x8
Hadamards 64 more) and 12 for the group sum: 316 (380), 49 times.  At 10 bits, without dot4: 144
sample offsets, per dx 12 x 4 x 8 multiply-adds + 48 shifts = 432.  Roof: 256 CUs x 4 SIMDs x 32
lanes/clk x 2.4 GHz (tools/merge_probe.py's).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd"), os.path.join(ROOT, "oracle")]

W, H = 1920, 1080
VALU_ROOF = 256 * 4 * 32 * 2.4e9   # lane-ops/s
WARM, ROUNDS = 3, 12


def frame_jobs():
    from nnfme import synth
    return synth.make_ctu_jobs(np.random.default_rng(7), W, H, 423, 4, [0, 1, 2, 3], [0])


def lane_ops(jobs, use_hadamard, bit_depth):
    from nnfme.abi import JOB_LOSSLESS
    units = (jobs["w"].astype(np.int64) // 4) * (jobs["h"] // 4)
    had8 = (((jobs["w"] | jobs["h"]) & 7) == 0) & bool(use_hadamard) & ((jobs["flags"] & JOB_LOSSLESS) == 0)
    first = 36 + 7 * 192 if bit_depth == 8 else 144 + 7 * 432
    per_unit = first + 49 * (316 + np.where(had8, 64, 0))
    return int((units * per_unit).sum())


def baseline_tasks(jobs):
    """49 fme_pe_tasks per uni-pred, unkeyed job: position i of job k at row 49 k + i."""
    from nnfme import merge, surface
    from nnfme.abi import JOB_BIPRED, JOB_LOSSLESS
    sel = np.flatnonzero((jobs["key_offset"] < 0) & ((jobs["flags"] & JOB_BIPRED) == 0))
    j = jobs[sel]
    t = np.zeros((len(j), surface.POINTS), merge.PE_TASK_DTYPE)
    for f in ("x", "y", "w", "h", "org_id"):
        t[f] = j[f][:, None]
    t["cu_x"] = (j["x"] // 64 * 64)[:, None]
    t["cu_y"] = (j["y"] // 64 * 64)[:, None]
    t["flags"] = (1 | np.where(j["flags"] & JOB_LOSSLESS, merge.PE_LOSSLESS, 0))[:, None]
    t["ref_id"][:, :, 0] = j["ref_id"][:, None]
    dx, dy = surface.offset(np.arange(surface.POINTS))
    t["mv"][:, :, 0, 0] = 4 * j["mv_x"][:, None].astype(np.int64) + dx[None, :]
    t["mv"][:, :, 0, 1] = 4 * j["mv_y"][:, None].astype(np.int64) + dy[None, :]
    return sel, t.reshape(-1)


def probe(jobs, bit_depth):
    import torch
    from nnfme import merge, surface, synth
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=0, use_hadamard=1, bit_depth=bit_depth)
    try:
        for k, t in zip(range(5), (7, 6, 5, 4, 0)):
            ctx.set_picture(k, synth.synth_luma(W, H, t) if bit_depth == 8 else synth.synth_luma_hbd(W, H, t, bit_depth))
        ctx.set_lambda(0, synth.LDP_LAMBDA[22][1])
        n = len(jobs)
        sel, tasks = baseline_tasks(jobs)
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        d_surf = torch.zeros(98 * n, dtype=torch.int32, device="cuda")
        d_pick = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        d_tasks = torch.from_numpy(tasks.view(np.uint8)).cuda()
        d_dist = torch.zeros(len(tasks), dtype=torch.int32, device="cuda")
        ctx.set_profiling(True)
        ms_s, ms_b = [], []
        for _ in range(WARM + ROUNDS):
            surface.cost_surface_device(ctx, d_jobs, None, d_surf, d_pick, n)
            ms_s.append(surface.cost_surface_last_ms(ctx))
            merge.pred_error_device(ctx, d_tasks, d_dist, len(tasks))
            ms_b.append(merge.pred_error_last_ms(ctx))
        assert surface.cost_surface_invalid_count(ctx) == 0 and merge.pred_error_invalid_count(ctx) == 0
        ms_s, ms_b = ms_s[WARM:], ms_b[WARM:]
        surf = d_surf.cpu().numpy().view(surface.SURFACE_DTYPE)
        base = d_dist.cpu().numpy().view(np.uint32).reshape(-1, surface.POINTS)
        same = float((surf["dist"][sel] == base).mean())
        med_s, med_b = float(np.median(ms_s)), float(np.median(ms_b))
        scale = n / len(sel)   # the baseline on the same number of jobs
        ops = lane_ops(jobs, 1, bit_depth)
        print(json.dumps({
            "probe": "k_cost_surface", "bit_depth": bit_depth, "jobs": n, "ms_median": round(med_s, 4),
            "ms_min": round(min(ms_s), 4), "ms_max": round(max(ms_s), 4), "jobs_per_s": round(n / (med_s * 1e-3)),
            "baseline": "fme_pred_error_device, 49 tasks per job", "baseline_jobs": int(len(sel)),
            "baseline_ms_median": round(med_b, 4), "baseline_ms_min": round(min(ms_b), 4),
            "baseline_ms_max": round(max(ms_b), 4), "baseline_over_surface": round(med_b * scale / med_s, 3),
            "dist_words_equal_to_baseline": round(same, 6), "lane_ops": ops,
            "valu_roof_fraction": round(ops / (med_s * 1e-3) / VALU_ROOF, 4)}), flush=True)
    finally:
        ctx.close()


def main():
    jobs = frame_jobs()
    for bd in (8, 10):
        probe(jobs, bd)


if __name__ == "__main__":
    main()
