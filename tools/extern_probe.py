#!/usr/bin/env python3
"""External-predictor timing probe (include/fme_extern.h).

One synthetic 1080p LDP frame's jobs (synth.make_ctu_jobs, 423 calls per CTU and reference, 4
references: 862,920 jobs, QP 22, the c3 batch of bench.py) resident on the device, one batch per call,
in one process.  Every arm is timed with a pair of HIP events on its stream and a synchronisation
after each call; after WARM warm-up calls the medians and extremes of ROUNDS calls are printed.

Arms every build can run (--lib: another build of libfme_amd.so, the parent commit's):
  ordinary        fme_refine_device alone;
  direct          fme_refine_direct_device alone;
  old_route       the only way to the NN inputs without fme_nn_inputs: an ordinary batch, the D2H of
                  the 64-byte records into pinned memory (device ms), then dataset.nn_inputs on the
                  host (wall ms, a few rounds: it is seconds long).
Arms of a build with the fme_extern.h entry points:
  inputs          fme_nn_inputs_device, and its phases with profiling on (EMI, rows, whole batch);
  at_rows/at_none fme_refine_at_device with the rows of the inputs batch / with rows == NULL, and the
                  evaluation kernel's share with profiling on;
  run_mlp         predictor.run with a small torch MLP (11 -> 64 -> 49) as one stream-ordered step.
The rows of the inputs batch must equal rows built from the ordinary batch's records, and with the
ordinary run's classes fme_refine_at_device must give the direct batch's records but for the status:
checked once.  One JSON line; no figure is compared against a target.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm16.9-nn_fme_amd")]

W, H, QP = 1920, 1080, 22
WARM, ROUNDS, PHASE_ROUNDS, HOST_ROUNDS = 4, 24, 8, 2


def frame_jobs():
    from nnfme import synth
    return synth.make_ctu_jobs(np.random.default_rng(7), W, H, 423, 4, [0, 1, 2, 3], [0])


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libfme_amd.so")
    ap.add_argument("--bit-depth", type=int, default=8)
    ap.add_argument("--no-host", action="store_true", help="skip the host half of old_route")
    args = ap.parse_args()
    import torch
    from nnfme import dataset, direct, predictor, synth
    from nnfme.abi import RESULT_DTYPE
    from nnfme.runtime import FmeContext, FmeError

    jobs = frame_jobs()
    n = len(jobs)
    ctx = FmeContext(nn_mode=1, use_hadamard=1, qp=QP, fast_inter_mode=1, bit_depth=args.bit_depth, lib_path=args.lib)
    out = {"probe": "extern", "lib": args.lib or "tree", "bit_depth": args.bit_depth, "jobs": n}
    try:
        have_extern = True
        try:
            predictor.bind(ctx.lib)
        except FmeError:
            have_extern = False
        for k, t in zip(range(5), (7, 6, 5, 4, 0)):
            ctx.set_picture(k, synth.synth_luma(W, H, t) if args.bit_depth == 8 else synth.synth_luma_hbd(W, H, t, args.bit_depth))
        for lid, lam in enumerate(synth.LDP_LAMBDA[QP]):
            ctx.set_lambda(lid, lam)
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        d_ord, d_dir, d_at, d_rows = (torch.zeros(n * 64, dtype=torch.uint8, device="cuda") for _ in range(4))
        d_cls = torch.zeros(n, dtype=torch.uint8, device="cuda")
        h_res = torch.zeros(n * 64, dtype=torch.uint8).pin_memory()
        s = torch.cuda.Stream()

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            call()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b)

        def rounds(call, before=None):
            ms = []
            for _ in range(WARM + ROUNDS):
                if before:
                    before()
                ms.append(timed(call))
            assert ctx.refine_status() == 0
            return stats(ms[WARM:])

        def ordinary():
            ctx.refine_device(d_jobs.data_ptr(), d_ord.data_ptr(), n, s.cuda_stream)

        def directly():
            direct.refine_direct_device(ctx, d_jobs, d_dir, n, s.cuda_stream)

        def download():
            ctx.download_device(d_ord.data_ptr(), h_res.data_ptr(), n * 64, 0, s.cuda_stream)

        out["ordinary_ms"] = rounds(ordinary, ctx.nn_reset)
        out["direct_ms"] = rounds(directly, ctx.nn_reset)
        out["old_route_d2h_ms"] = rounds(download)
        ro = h_res.numpy().view(RESULT_DTYPE).copy()
        if not args.no_host:
            wall = []
            for _ in range(HOST_ROUNDS):
                t0 = time.perf_counter()
                e, c, ph, pw, _ = dataset.nn_inputs(jobs, ro, None)
                wall.append(1e3 * (time.perf_counter() - t0))
            out["old_route_host_fill_wall_ms"] = stats(wall)
        if have_extern:
            def inputs():
                predictor.nn_inputs_device(ctx, d_jobs, d_rows, n, s.cuda_stream)

            def at_rows():
                predictor.refine_at_device(ctx, d_jobs, d_rows, d_cls, d_at, n, s.cuda_stream)

            def at_none():
                predictor.refine_at_device(ctx, d_jobs, None, d_cls, d_at, n, s.cuda_stream)

            out["inputs_ms"] = rounds(inputs, ctx.nn_reset)
            rows = d_rows.cpu().numpy().view(predictor.NN_ROW_DTYPE)
            want, _ = predictor.rows_numpy(jobs, ro, None)
            assert rows.tobytes() == want.tobytes(), "rows differ from the ordinary batch's records"
            d_cls.copy_(torch.from_numpy(ro["nn_class"].copy()))
            torch.cuda.synchronize()
            out["at_rows_ms"] = rounds(at_rows)
            with_rows = d_at.cpu().numpy().view(RESULT_DTYPE).copy()
            out["at_none_ms"] = rounds(at_none)
            assert predictor.refine_at_status(ctx) == 0
            rd, ra = d_dir.cpu().numpy().view(RESULT_DTYPE).copy(), d_at.cpu().numpy().view(RESULT_DTYPE)
            assert ra.tobytes() == with_rows.tobytes(), "records with and without rows differ"
            rd["status"] = direct.RES_NN_DIRECT | predictor.RES_NN_EXTERN
            assert ra.tobytes() == rd.tobytes(), "fme_refine_at with the net's classes differs from the direct batch"

            torch.manual_seed(0)
            mlp = torch.nn.Sequential(torch.nn.Linear(11, 64), torch.nn.ReLU(), torch.nn.Linear(64, 49)).cuda().eval()

            def run():
                predictor.run(ctx, d_jobs, mlp, d_rows, d_cls, d_at, s)

            out["run_mlp_ms"] = rounds(run, ctx.nn_reset)
            assert predictor.refine_at_status(ctx) == 0
            out["run_mlp_classes"] = int(len(np.unique(d_cls.cpu().numpy())))
            ctx.set_profiling(True)
            for name, call in (("inputs", inputs), ("at_rows", at_rows), ("at_none", at_none)):
                ph = []
                for _ in range(2 + PHASE_ROUNDS):
                    call()
                    ph.append(predictor.last_ms(ctx))
                for k in predictor.LAST_MS_NAMES:
                    out[f"{name}_phase_{k}_ms"] = stats([p[k] for p in ph[2:]])
            ctx.set_profiling(False)
    finally:
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
