#!/usr/bin/env python3
"""The GPU parts of the timing probes under tools/, without their one-core CPU comparisons, plus
the 10-bit forms that tools/mc_probe.py and tools/pred_inter_probe.py lack.
usage: python tools/pred_family_probe.py merge|skip|mc|pi   (tools/pred_family_ab.sh runs them A/B)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]


def merge():
    import merge_probe as m
    tasks = m.frame_tasks(np.random.default_rng(7))
    m.gpu_rate(tasks, 8)
    m.gpu_rate(tasks, 10)


def skip():
    import skip_probe as s
    from nnfme import skip as sk, synth
    reqs = s.frame_requests(np.random.default_rng(7))
    params = sk.make_params(synth.LDP_LAMBDA[22][1], (2.0 ** (-1.0 / 3.0), 2.0 ** (-1.0 / 3.0)))
    s.gpu_rate(reqs, params, 8)
    s.gpu_rate(reqs, params, 10)


def mc():
    """k_mc on a whole 1080p partition (30 % bi-pred), kernel ms from the library's events."""
    import torch
    from nnfme import synth
    from nnfme.runtime import FmeContext
    W, H = 1920, 1080
    dev = torch.device("cuda", 0)
    jobs = synth.make_mc_partition(np.random.default_rng(5), W, H, [0, 1, 2, 3], bi_frac=0.3, mv_amp=64)
    for bd in (8, 10):
        ctx = FmeContext(nn_mode=0, bit_depth=bd)
        for k in range(4):
            cb, cr = synth.synth_chroma(W, H, k)
            if bd == 8:
                ctx.set_picture_yuv(k, synth.synth_luma(W, H, k), cb, cr)
            else:
                ctx.set_picture_yuv(k, synth.synth_luma_hbd(W, H, k, bit_depth=10), cb.astype(np.uint16) << 2,
                                    cr.astype(np.uint16) << 2)
        tdt = torch.uint8 if bd == 8 else torch.int16
        dy = torch.zeros((H, W), dtype=tdt, device=dev)
        dcb = torch.zeros((H // 2, W // 2), dtype=tdt, device=dev)
        dcr = torch.zeros_like(dcb)
        dj = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        ctx.set_profiling(True)
        ms = []
        for _ in range(43):
            ctx.motion_compensate_device(dj.data_ptr(), len(jobs), dy.data_ptr(), W, dcb.data_ptr(), dcr.data_ptr(),
                                         W // 2, W, H, s)
            ms.append(ctx.mc_last_ms())
        assert ctx.mc_invalid_count() == 0
        ms = ms[3:]
        print(json.dumps({"probe": "k_mc", "bit_depth": bd, "jobs": len(jobs), "ms_median": round(float(np.median(ms)), 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}), flush=True)
        ctx.close()


def pi():
    """tools/pred_inter_probe.py's P and B frames at bit depth 10: the phases hold the AMVP template
    costs (k_amvp_sad) and the bi-pred key builds (k_bi_key)."""
    from nnfme import synth
    from nnfme.runtime import FmeContext
    W, H = 1920, 1080
    pics = {i: synth.synth_luma_hbd(W, H, t, bit_depth=10) for i, t in zip(range(6), (7, 6, 5, 4, 0, 3))}
    reqs = synth.make_pu_requests(np.random.default_rng(2), W, H, org_id=4, ref_ids=[0, 1, 2, 3], lambda_id=0, max_depth=3)
    ctx = FmeContext(nn_mode=1, qp=22, fast_inter_mode=1, max_jobs=4 * len(reqs), bit_depth=10)
    for k, v in pics.items():
        ctx.set_picture(k, v)
    for lid, lam in enumerate(synth.LDP_LAMBDA[22]):
        ctx.set_lambda(lid, lam)
    reqs_b = synth.make_pu_requests_b(np.random.default_rng(3), W, H, org_id=4, l0=[(0, 1), (1, 2)],
                                      l1=[(5, -1), (2, -2)], lambda_id=0, max_depth=3)
    for name, call, r in (("pred_inter_p", ctx.pred_inter_p, reqs), ("pred_inter_b", ctx.pred_inter_b, reqs_b)):
        call(r)   # warm-up
        ts, ph = [], []
        for _ in range(5):
            ctx.pred_inter_reset()
            t0 = time.perf_counter()
            call(r)
            ts.append((time.perf_counter() - t0) * 1e3)
            ph.append(ctx.pred_inter_phases())
        print(json.dumps({"probe": name, "bit_depth": 10, "requests": len(r), "ms_median": round(float(np.median(ts)), 2),
                          "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2),
                          "phases_ms_median": {k: round(float(np.median([p[k] for p in ph])), 3) for k in ph[0]}}),
              flush=True)


if __name__ == "__main__":
    {"merge": merge, "skip": skip, "mc": mc, "pi": pi}[sys.argv[1]]()
