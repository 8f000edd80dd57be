#!/usr/bin/env python3
"""NN-direct timing probe (include/fme_direct.h).

One synthetic 1080p LDP frame's jobs (synth.make_ctu_jobs, 423 calls per CTU and reference, 4
references: 862,920 jobs, QP 22, the c3 batch of bench.py) resident on the device, refined as one
batch per call, in one process:

  ordinary   fme_refine_device alone, a device synchronisation after every batch: the arm a library
             without the direct entry points (--lib, the parent commit's build) can run too, so the
             ordinary path of two builds can be compared;
  alternate  fme_refine_device and fme_refine_direct_device in turn on one stream.

Each batch is timed with a pair of HIP events on its stream; after WARM warm-up batches per arm the
medians and extremes of ROUNDS batches are printed, with the ratio direct / ordinary from the
alternating rounds.  Then, with profiling on, the direct batch's three phases (EMI kernel, class
kernel, evaluation kernel) and the whole batch from fme_refine_direct_last_ms.  One JSON line; no
figure is compared against a target.  The direct records' classes must equal the ordinary ones'
(the same job stream from the same state), which the probe checks on the last round.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd")]

W, H, QP = 1920, 1080, 22
WARM, ROUNDS, PHASE_ROUNDS = 4, 24, 8


def frame_jobs():
    from nnfme import synth
    return synth.make_ctu_jobs(np.random.default_rng(7), W, H, 423, 4, [0, 1, 2, 3], [0])


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libfme_amd.so (ordinary arm only when it lacks the direct entry points)")
    ap.add_argument("--bit-depth", type=int, default=8)
    args = ap.parse_args()
    import torch
    from nnfme import direct, synth
    from nnfme.abi import RESULT_DTYPE
    from nnfme.runtime import FmeContext, FmeError

    jobs = frame_jobs()
    n = len(jobs)
    ctx = FmeContext(nn_mode=1, use_hadamard=1, qp=QP, fast_inter_mode=1, bit_depth=args.bit_depth, lib_path=args.lib)
    out = {"probe": "direct", "lib": args.lib or "tree", "bit_depth": args.bit_depth, "jobs": n}
    try:
        have_direct = True
        try:
            direct.bind(ctx.lib)
        except FmeError:
            have_direct = False
        for k, t in zip(range(5), (7, 6, 5, 4, 0)):
            ctx.set_picture(k, synth.synth_luma(W, H, t) if args.bit_depth == 8 else synth.synth_luma_hbd(W, H, t, args.bit_depth))
        for lid, lam in enumerate(synth.LDP_LAMBDA[QP]):
            ctx.set_lambda(lid, lam)
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        d_ord = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_dir = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            call()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b)

        def ordinary():
            ctx.refine_device(d_jobs.data_ptr(), d_ord.data_ptr(), n, s.cuda_stream)

        def directly():
            direct.refine_direct_device(ctx, d_jobs, d_dir, n, s.cuda_stream)

        ms = [timed(ordinary) for _ in range(WARM + ROUNDS)][WARM:]
        assert ctx.refine_status() == 0
        out["ordinary_alone_ms"] = stats(ms)
        if have_direct:
            ms_o, ms_d = [], []
            for _ in range(WARM + ROUNDS):
                ctx.nn_reset()
                ms_o.append(timed(ordinary))
                ctx.nn_reset()
                ms_d.append(timed(directly))
            assert ctx.refine_status() == 0
            ms_o, ms_d = ms_o[WARM:], ms_d[WARM:]
            out["ordinary_alternating_ms"] = stats(ms_o)
            out["direct_ms"] = stats(ms_d)
            out["direct_over_ordinary"] = round(float(np.median(ms_d) / np.median(ms_o)), 4)
            ro, rd = d_ord.cpu().numpy().view(RESULT_DTYPE), d_dir.cpu().numpy().view(RESULT_DTYPE)
            for f in ("mv_int_x", "mv_int_y", "c", "emi", "n_emi", "nn_class"):
                assert np.array_equal(ro[f], rd[f]), f
            assert np.array_equal(rd["status"], ro["status"] | direct.RES_NN_DIRECT)
            out["direct_frac_cost_le_shipped"] = round(float((rd["frac_cost"] <= ro["frac_cost"]).mean()), 4)
            out["direct_frac_cost_eq_shipped"] = round(float((rd["frac_cost"] == ro["frac_cost"]).mean()), 4)
            ctx.set_profiling(True)
            ph = []
            for _ in range(2 + PHASE_ROUNDS):
                directly()
                ph.append(direct.last_ms(ctx))
            ctx.set_profiling(False)
            for name in direct.LAST_MS_NAMES:
                out[f"phase_{name}_ms"] = stats([p[name] for p in ph[2:]])
    finally:
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
