#!/usr/bin/env python3
"""Drop-in call latency breakdown: host wall time per fme_frac_dif_single / fme_nn_pred_single call
(through ctypes, so a little above the C++ figure) against the server's device service time
(fme_single_last_device_us): the difference is host + PCIe + polling.

usage: python tools/single_probe.py [calls] [--bit-depth {8,10}]

--bit-depth 10: a 10-bit context and synth_luma_hbd pictures (the main10 configurations).  Only the
Python ABI is used, so the same file measures any build of the library ($FME_LIB_PATH)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm16.9-nn_fme_amd"))


def main():
    from nnfme import synth, weights
    from nnfme.runtime import FmeContext
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("calls", nargs="?", type=int, default=300)
    ap.add_argument("--bit-depth", type=int, choices=(8, 10), default=8)
    args = ap.parse_args()
    calls, bd = args.calls, args.bit_depth
    ctx = FmeContext(nn_mode=1, qp=22, bit_depth=bd)
    ctx.load_nn(weights.load_weights(22))
    W, H, pad = 416, 240, 80
    luma = synth.synth_luma if bd == 8 else (lambda w, h, t: synth.synth_luma_hbd(w, h, t, bd))
    pic = np.pad(luma(W, H, 1).astype(np.int16), pad, mode="edge")
    org = luma(W, H, 2).astype(np.int16)
    print(f"bit depth {bd}, {calls} calls per shape", flush=True)
    rng = np.random.default_rng(3)
    ml = 65536.0 * np.sqrt(synth.LDP_LAMBDA[22][0])
    for (w, h) in ((8, 8), (16, 16), (64, 64)):
        wall, dev, ph = [], [], []
        for i in range(calls):
            x, y = 4 * int(rng.integers(0, (W - w) // 4)), 4 * int(rng.integers(0, (H - h) // 4))
            key = org[y:y + h, x:x + w]
            mv = tuple(int(v) for v in rng.integers(-8, 9, 2))
            mvp = tuple(int(v) for v in rng.integers(-16, 17, 2))
            t0 = time.perf_counter()
            ctx.frac_dif_single(key, pic, (y + pad, x + pad), mv, mvp, ml)
            wall.append(time.perf_counter() - t0)
            p = ctx.single_last_device_us(phases=True)
            dev.append(p[0])
            ph.append(p[1:])
        m = np.median(np.array(ph[1:]), axis=0)
        print(f"frac_dif {w}x{h}: wall {np.median(wall[1:]) * 1e6:.2f} us, device {np.median(dev[1:]):.2f} us "
              f"(payload {m[0]:.2f}, first stage {m[1]:.2f}, half dist {m[2]:.2f}, quarter dist {m[3]:.2f})", flush=True)
    wall, dev, net = [], [], []
    for i in range(calls):
        e = rng.integers(0, 5000, 8).astype(np.uint32)
        t0 = time.perf_counter()
        ctx.nn_pred_single(e, int(rng.integers(0, 5000)), 8, 8)
        wall.append(time.perf_counter() - t0)
        p = ctx.single_last_device_us(phases=True)
        dev.append(p[0])
        net.append(p[1:3])
    # the NN marks: shader-clock cycles of the net (reported through the 100 MHz wall scale) and
    # its wall time, so their ratio is the shader clock while the server runs
    cyc, nus = np.median(np.array(net[1:]), axis=0)
    print(f"nn_pred: wall {np.median(wall[1:]) * 1e6:.2f} us, device {np.median(dev[1:]):.2f} us, "
          f"net {nus:.2f} us = {cyc * 100:.0f} shader cycles ({cyc * 100 / max(nus, 1e-3):.0f} MHz)", flush=True)


if __name__ == "__main__":
    main()
