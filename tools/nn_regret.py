#!/usr/bin/env python3
"""What the NN's pick and the two-stage search's pick cost against the best of the 49 quarter-pel
positions (include/fme_surface.h).

One synthetic 1080p LDP frame's jobs (synth.make_ctu_jobs: 862,920 jobs), refined with NN on by
each of the four per-QP weight sets (QP 22 / 27 / 32 / 37, that QP's lambda); then the cost surface
centred on each job's mv_int with the job's nn_class as the probe.  Per QP one JSON line: the mean
and the 99th percentile of cost[nn_class] - min and of frac_cost - min, the share of jobs where
each is zero, and the mean minimum for scale.  A finding, not a gate.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd"), os.path.join(ROOT, "oracle")]

W, H = 1920, 1080


def main():
    from nnfme import surface, synth
    from nnfme.runtime import FmeContext
    jobs = synth.make_ctu_jobs(np.random.default_rng(7), W, H, 423, 4, [0, 1, 2, 3], [0])
    pics = {k: synth.synth_luma(W, H, t) for k, t in zip(range(5), (7, 6, 5, 4, 0))}
    for qp in (22, 27, 32, 37):
        ctx = FmeContext(device=0, use_hadamard=1, nn_mode=1, qp=qp, fast_inter_mode=1)
        try:
            for k, v in pics.items():
                ctx.set_picture(k, v)
            ctx.set_lambda(0, synth.LDP_LAMBDA[qp][1])
            res = ctx.refine(jobs)
            probes = np.stack([res["nn_class"], np.full(len(jobs), surface.NO_PROBE, np.uint8)], axis=1)
            _, pick = surface.cost_surface(ctx, surface.jobs_at_results(jobs, res), probes, surface=False)
        finally:
            ctx.close()
        lo = pick["min_cost"].astype(np.int64)
        nn = pick["probe_cost"][:, 0].astype(np.int64) - lo
        se = res["frac_cost"].astype(np.int64) - lo
        assert (nn >= 0).all() and (se >= 0).all() and (pick["status"] == 0).all()
        print(json.dumps({
            "probe": "nn_regret", "qp": qp, "jobs": len(jobs), "min_cost_mean": round(float(lo.mean()), 2),
            "nn_regret_mean": round(float(nn.mean()), 3), "nn_regret_p99": int(np.percentile(nn, 99)),
            "nn_regret_zero_share": round(float((nn == 0).mean()), 4),
            "search_regret_mean": round(float(se.mean()), 3), "search_regret_p99": int(np.percentile(se, 99)),
            "search_regret_zero_share": round(float((se == 0).mean()), 4),
            "nn_equals_search_share": round(float((nn == se).mean()), 4)}), flush=True)


if __name__ == "__main__":
    main()
