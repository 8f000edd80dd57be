#!/usr/bin/env python3
"""Candidate-set refinement timing and regret probe (include/fme_among.h).

One synthetic 1080p LDP frame's jobs (synth.make_ctu_jobs, 423 calls per CTU and reference, 4
references: 862,920 jobs, QP 22, the c3 batch of bench.py) resident on the device, one batch per call,
all arms in one process.  Every batch is timed with a pair of HIP events on its stream and a
synchronisation after each call: ROUNDS timed batches after WARM warm-ups make one run, RUNS runs per
library, this tree and the build given with --lib (the parent commit's) alternating.  Per arm the
median of each run and the range of the runs' medians are printed.

Undisturbed arms, both libraries: the ordinary batch, the direct batch, the at batch with rows.
New arms, this tree: the among batch with rows and the top-K batch at k = 1, 2, 4, 8, and
fme_among_last_ms's phases for both.
Baseline of the new arms, both libraries: the only earlier route to the same records, k
fme_refine_at_mv_device batches with rows and the elementwise minimum in torch on the same stream.
The among batch's records are checked once against that baseline's (cost and class of the minimum).

--regret: per QP the mean, p99 and share 0 of frac_cost - min over the 49-point surface for the net's
class alone (the direct batch) and for top-2, top-4 and top-8 of the shipped weights.  The frame is
synthetic: it is not the content the weights were trained on.
One JSON line; no figure is compared against a target.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd")]

W, H, QP = 1920, 1080, 22
WARM, ROUNDS, RUNS, PHASE_ROUNDS = 4, 24, 3, 8
KS = (1, 2, 4, 8)


def frame_jobs():
    from nnfme import synth
    return synth.make_ctu_jobs(np.random.default_rng(7), W, H, 423, 4, [0, 1, 2, 3], [0])


def summary(medians):
    return {"run_medians": [round(m, 4) for m in medians], "min": round(min(medians), 4), "max": round(max(medians), 4)}


def open_ctx(lib, qp, bit_depth, max_jobs):
    from nnfme import synth
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=1, use_hadamard=1, qp=qp, fast_inter_mode=1, bit_depth=bit_depth, lib_path=lib,
                     max_jobs=max_jobs)
    for k, t in zip(range(5), (7, 6, 5, 4, 0)):
        ctx.set_picture(k, synth.synth_luma(W, H, t) if bit_depth == 8 else synth.synth_luma_hbd(W, H, t, bit_depth))
    for lid, lam in enumerate(synth.LDP_LAMBDA[qp]):
        ctx.set_lambda(lid, lam)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libfme_amd.so (the parent commit's)")
    ap.add_argument("--bit-depth", type=int, default=8)
    ap.add_argument("--regret", action="store_true", help="the regret columns instead of the timing arms")
    args = ap.parse_args()
    import torch
    from nnfme import among, direct, predictor, surface
    from nnfme.abi import MV_RESULT_DTYPE, RESULT_DTYPE

    jobs = frame_jobs()
    n = len(jobs)
    out = {"probe": "among", "lib": args.lib or None, "bit_depth": args.bit_depth, "jobs": n}
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    s = torch.cuda.Stream()

    if args.regret:
        for qp in (22, 27, 32, 37):
            ctx = open_ctx(None, qp, args.bit_depth, n)
            try:
                ref = ctx.refine(jobs)
                _, pick = surface.cost_surface(ctx, surface.jobs_at_results(jobs, ref), surface=False, pick=True)
                least = pick["min_cost"].astype(np.int64)
                d_res = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
                for k in KS:
                    ctx.nn_reset()
                    among.refine_topk_device(ctx, d_jobs, d_res, k, None, None, n, s.cuda_stream)
                    s.synchronize()
                    assert ctx.refine_status() == 0 and among.refine_among_status(ctx) == 0
                    r = d_res.cpu().numpy().view(RESULT_DTYPE)["frac_cost"].astype(np.int64) - least
                    assert (r >= 0).all()
                    out[f"qp{qp}_top{k}"] = {"mean": round(float(r.mean()), 2), "p99": int(np.percentile(r, 99)),
                                            "share0": round(float((r == 0).mean()), 4)}
            finally:
                ctx.close()
        print(json.dumps(out), flush=True)
        return

    libs = {"tree": None}
    if args.lib:
        libs["other"] = args.lib
    ctxs = {name: open_ctx(path, QP, args.bit_depth, n) for name, path in libs.items()}
    try:
        d_res, d_rows = (torch.zeros(n * 64, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_mv = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in range(max(KS))]
        d_best = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_cand = torch.zeros(n * max(KS), dtype=torch.uint8, device="cuda")
        d_cost = torch.zeros(n * max(KS), dtype=torch.int32, device="cuda")

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            call()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b)

        def one_run(ctx, call, before=None):
            ms = []
            for _ in range(WARM + ROUNDS):
                if before:
                    before()
                ms.append(timed(call))
            assert ctx.refine_status() == 0
            return float(np.median(ms[WARM:]))

        # the rows and the net's 8 best classes, once (this tree), shared by every arm
        tree = ctxs["tree"]
        tree.nn_reset()
        predictor.nn_inputs_device(tree, d_jobs, d_rows, n, s.cuda_stream)
        among.nn_rank_device(tree, d_rows, d_cand, max(KS), n, s.cuda_stream)
        s.synchronize()
        top8 = d_cand.cpu().numpy().reshape(n, max(KS))
        d_list = {k: torch.from_numpy(np.ascontiguousarray(top8[:, :k])).cuda() for k in KS}
        d_col = [torch.from_numpy(np.ascontiguousarray(top8[:, q])).cuda() for q in range(max(KS))]

        def arms(name, ctx):
            def ordinary():
                ctx.refine_device(d_jobs.data_ptr(), d_res.data_ptr(), n, s.cuda_stream)

            def directly():
                direct.refine_direct_device(ctx, d_jobs, d_res, n, s.cuda_stream)

            def at_rows():
                predictor.refine_at_device(ctx, d_jobs, d_rows, d_col[0], d_res, n, s.cuda_stream)

            def baseline(k):
                def call():
                    for q in range(k):
                        predictor.refine_at_mv_device(ctx, d_jobs, d_rows, d_col[q], d_mv[q], n, s.cuda_stream)
                    with torch.cuda.stream(s):    # the elementwise minimum: the first of least cost
                        cost = torch.stack([(t.view(torch.int32).view(n, 4)[:, 1].to(torch.int64) & 0xFFFFFFFF) for t in d_mv[:k]])
                        best = cost.argmin(dim=0)
                        recs = torch.stack([t.view(n, 16) for t in d_mv[:k]])
                        d_best.view(n, 16).copy_(recs[best, torch.arange(n, device="cuda")])
                return call

            a = {"ordinary": (ordinary, ctx.nn_reset), "direct": (directly, ctx.nn_reset), "at_rows": (at_rows, None)}
            for k in KS:
                a[f"baseline_k{k}"] = (baseline(k), None)
            if name == "tree":
                for k in KS:
                    a[f"among_rows_k{k}"] = ((lambda k=k: among.refine_among_mv_device(ctx, d_jobs, d_rows, d_list[k], k, d_mv[0],
                                                                                      None, n, s.cuda_stream)), None)
                    a[f"topk_k{k}"] = ((lambda k=k: among.refine_topk_mv_device(ctx, d_jobs, d_mv[0], k, None, None, n,
                                                                               s.cuda_stream)), ctx.nn_reset)
            return a

        all_arms = {name: arms(name, ctx) for name, ctx in ctxs.items()}
        medians = {name: {arm: [] for arm in a} for name, a in all_arms.items()}
        for _ in range(RUNS):                      # the libraries alternate within every run
            for arm in all_arms["tree"]:
                for name, ctx in ctxs.items():
                    if arm in all_arms[name]:
                        call, before = all_arms[name][arm]
                        medians[name][arm].append(one_run(ctx, call, before))
        for name in medians:
            out[name] = {arm: summary(m) for arm, m in medians[name].items()}

        # the among batch against the baseline, once: the same minimum and the same class (k = 8)
        all_arms["tree"]["baseline_k8"][0]()
        among.refine_among_mv_device(tree, d_jobs, d_rows, d_list[8], 8, d_mv[0], d_cost, n, s.cuda_stream)
        s.synchronize()
        base, got = d_best.cpu().numpy().view(MV_RESULT_DTYPE), d_mv[0].cpu().numpy().view(MV_RESULT_DTYPE)
        # (the baseline's cost is the tail's; the among batch picks by frac_cost: the classes may differ where the tail reorders)
        out["among_equals_baseline_class_share"] = round(float((base["nn_class"] == got["nn_class"]).mean()), 6)
        assert among.refine_among_status(tree) == 0

        tree.set_profiling(True)
        for k in KS:
            for arm in (f"among_rows_k{k}", f"topk_k{k}"):
                call, before = all_arms["tree"][arm]
                ph = []
                for _ in range(2 + PHASE_ROUNDS):
                    if before:
                        before()
                    call()
                    ph.append(among.last_ms(tree))
                out[f"{arm}_phases_ms"] = {p: round(float(np.median([x[p] for x in ph[2:]])), 4) for p in among.LAST_MS_NAMES}
        tree.set_profiling(False)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
