#!/usr/bin/env python3
"""Skip-check timing probe (include/fme_skip.h).

One 1080p frame's worth of 2Nx2N CUs at depths 0-3 (every 64 / 32 / 16 / 8 CU that lies inside the
picture: 42,900 CUs), five merge candidates each, all evaluated, as one fme_skip_estimate batch of
214,500 SSE tasks: the k_pred_sse time from fme_pred_sse_last_ms and the end-to-end time of
fme_skip_estimate (expansion, upload, launch, download, host arithmetic), medians of 20 calls after
3 warm-ups with their range, at 8 and 10 bits; then the one-core rate of the reference composition
the fixtures use (oracle/_ref: Reference.mc of Y / Cb / Cr + the numpy SSE per task) on a 20,000-task
sample of the same list, where that library is built, compared with the GPU's values.  Prints one
JSON line per measurement.  No figure is compared against a target.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd"), os.path.join(ROOT, "oracle")]

W, H = 1920, 1080


def frame_requests(rng):
    from nnfme import skip, synth
    vx, vy = synth.motion_field(rng, (W + 63) // 64, (H + 63) // 64)   # one motion per CTU, full-pel
    field = np.rint(4.0 * np.stack([vx, vy], axis=-1))                  # [ctu_y, ctu_x, (hor, ver)] quarter-pel
    reqs = []
    for s in (64, 32, 16, 8):
        xs, ys = np.meshgrid(np.arange(0, W - s + 1, s), np.arange(0, H - s + 1, s))
        q = np.zeros(xs.size, skip.SKIP_REQ_DTYPE)
        q["x"], q["y"] = xs.reshape(-1), ys.reshape(-1)
        q["w"] = q["h"] = s
        reqs.append(q)
    q = np.concatenate(reqs)
    n = len(q)
    q["org_id"], q["n_cand"], q["cand_mask"] = 0, 5, 0x1F
    near = np.asarray(field)[q["y"] // 64, q["x"] // 64].astype(np.int64).reshape(n, 1, 1, 2)
    q["cand"]["inter_dir"] = rng.choice([1, 2, 3], size=(n, 5), p=[0.45, 0.2, 0.35])
    q["cand"]["ref_id"] = rng.integers(1, 4, (n, 5, 2))
    q["cand"]["mv"] = np.clip(near + rng.integers(-12, 13, (n, 5, 2, 2)), -32768, 32767)
    q["bits"] = rng.integers(1, 41, (n, 5))
    return q


def pictures(bit_depth):
    from nnfme import synth
    out = []
    for k in range(4):
        if bit_depth == 8:
            out.append((synth.synth_luma(W, H, k),) + tuple(synth.synth_chroma(W, H, k)))
        else:
            out.append((synth.synth_luma_hbd(W, H, k, bit_depth), synth.synth_luma_hbd(W // 2, H // 2, k, bit_depth, seed=42),
                        synth.synth_luma_hbd(W // 2, H // 2, k, bit_depth, seed=43)))
    return out


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def gpu_rate(reqs, params, bit_depth):
    from nnfme import skip
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=0, use_hadamard=1, bit_depth=bit_depth)
    try:
        for k, p in enumerate(pictures(bit_depth)):
            ctx.set_picture_yuv(k, *p)
        ctx.set_profiling(True)
        kern, wall = [], []
        for i in range(23):
            t0 = time.perf_counter()
            res = skip.skip_estimate(ctx, params, reqs)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(skip.pred_sse_last_ms(ctx))
        n_tasks = 5 * len(reqs)   # every request evaluates its five candidates
        k, w = stats(kern[3:]), stats(wall[3:])
        print(json.dumps({"probe": "fme_skip_estimate", "bit_depth": bit_depth, "requests": len(reqs), "tasks": n_tasks,
                          "runs": 20, "kernel_ms": k, "end_to_end_ms": w,
                          "tasks_per_s_kernel": round(n_tasks / (k["median"] * 1e-3)),
                          "tasks_per_s_end_to_end": round(n_tasks / (w["median"] * 1e-3))}), flush=True)
        return res
    finally:
        ctx.close()


def ref_rate(reqs, got, sample=4000):
    """sample requests (x 5 candidates) through Reference.mc + sse_numpy on one core."""
    from nnfme import skip
    from nnfme.abi import MC_JOB_DTYPE
    from oracle import REF_SO, Reference
    if not os.path.exists(REF_SO):
        print(json.dumps({"probe": "ref_composition", "skipped": "oracle/_ref is not built"}), flush=True)
        return
    ref = Reference()
    pics = pictures(8)
    for k, p in enumerate(pics):
        ref.set_picture_yuv(k, *p)
    idx = np.sort(np.random.default_rng(3).choice(len(reqs), sample, replace=False))
    tasks, first = skip.expand_requests(reqs[idx])
    jobs = np.zeros(len(tasks), MC_JOB_DTYPE)
    for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv", "flags"):
        jobs[f] = tasks[f]
    pred = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    out = np.zeros((len(tasks), 3), np.uint32)
    t0 = time.perf_counter()
    for i in range(len(tasks)):
        ref.mc(jobs[i:i + 1], *pred)
        out[i] = skip.block_sse(pics[0], pred, tasks[i], 8)
    dt = time.perf_counter() - t0
    print(json.dumps({"probe": "ref_composition", "tasks": len(tasks), "seconds": round(dt, 3),
                      "tasks_per_s": round(len(tasks) / dt),
                      "equal_to_gpu": bool(np.array_equal(out.reshape(sample, 5, 3), got["cand_sse"][idx]))}), flush=True)


def main():
    from nnfme import skip, synth
    reqs = frame_requests(np.random.default_rng(7))
    params = skip.make_params(synth.LDP_LAMBDA[22][1], (2.0 ** (-1.0 / 3.0), 2.0 ** (-1.0 / 3.0)))
    got8 = gpu_rate(reqs, params, 8)
    gpu_rate(reqs, params, 10)
    ref_rate(reqs, got8)


if __name__ == "__main__":
    main()
