#!/usr/bin/env python3
"""Generate tests/golden/*.npz — TEST INFRASTRUCTURE ONLY (run in the build container).

Expected outputs come from oracle/_ref/libhmref.so: the reference's own TLibCommon sources
(TComInterpolationFilter, TComRdCost, TComPicYuv, TComPrediction scratch planes) compiled
from /root/reference and driven in TEncSearch's order by oracle/ref_harness.cpp.  Every case
is also run through the plain-C oracle (fme_oracle.c); generation aborts on any mismatch.

Each fixture holds inputs and outputs only (data): pictures, lambdas, bi-pred key blocks,
jobs (fme_job records), results (fme_result records) and the configuration.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "hm16.9-nn_fme_amd")]

from oracle import Oracle, Reference  # noqa: E402
from nnfme import synth, weights  # noqa: E402
from nnfme.abi import JOB_BIPRED, JOB_EMI, JOB_LOSSLESS, JOB_NN_IN, TZ_RING, compare_results  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def edge_jobs(rng, width, height, n):
    """Jobs that hit the corners: search-range edges (< 8 EMI pushes), picture borders with MVs
    pointing outside (edge replication), the largest PUs."""
    sizes = [s for s in synth.ALL_PU_SIZES]
    picks = [sizes[i % len(sizes)] for i in range(n)]
    w = np.array([p[0] for p in picks])
    h = np.array([p[1] for p in picks])
    j = synth.make_jobs(rng, width, height, n, 4, [0, 1, 2], [0, 1, 2, 3], sizes=(w, h))
    for i in range(n):
        kind = i % 6
        if kind == 0:      # TZ best on the left/top range edge
            j["mv_x"][i] = j["lt_x"][i]
            j["mv_y"][i] = j["lt_y"][i]
        elif kind == 1:    # right/bottom edge
            j["mv_x"][i] = j["rb_x"][i]
            j["mv_y"][i] = j["rb_y"][i]
        elif kind == 2:    # PU at the top-left corner, MV far outside
            j["x"][i] = 0
            j["y"][i] = 0
            j["mv_x"][i] = max(int(j["lt_x"][i]), -60)
            j["mv_y"][i] = max(int(j["lt_y"][i]), -60)
        elif kind == 3:    # bottom-right corner
            j["x"][i] = (width - j["w"][i]) // 4 * 4
            j["y"][i] = (height - j["h"][i]) // 4 * 4
        elif kind == 4:    # degenerate range: a single column
            j["lt_x"][i] = j["rb_x"][i] = j["mv_x"][i]
        else:              # lossless CU (SAD in FracDIF)
            j["flags"][i] = JOB_EMI | JOB_LOSSLESS
    # the search range must contain the start point (xTZSearch invariant)
    return j


def build_case(name, seed, width, height, n_jobs, hadme, fen, nn_mode, qp, bipred=0.15, n_edge=96, net=None, gop="ldp",
               bit_depth=8):
    """bit_depth 10: the main10 configurations (cfg/encoder_lowdelay_P_main10.cfg:58): 16-bit
    pictures, _ref's TComInterpolationFilter / TComRdCost run with bitDepth 10.  The lambdas are the
    8-bit ones: HM scales the QP by 6 * (bitDepth - 8 - DISTORTION_PRECISION_ADJUSTMENT(bitDepth - 8))
    = 0 in the shipped build (TypeDef.h:140-143, FULL_NBIT 0), so lambda does not change."""
    rng = np.random.default_rng(seed)
    if bit_depth > 8:
        pics = {i: synth.synth_luma_hbd(width, height, i, bit_depth, seed=seed) for i in range(5)}
    else:
        pics = {i: synth.synth_luma(width, height, i, seed=seed) for i in range(5)}
    if gop == "ra":   # random-access GOP-8 lambdas (TEncSlice.cpp:246-325): entries POC 8, 4, 2, 1
        lambdas = np.array([synth.ra_lambda(qp, e) for e in range(4)], dtype=np.float64)
    else:
        lambdas = np.array(synth.LDP_LAMBDA[qp if qp in synth.LDP_LAMBDA else 22], dtype=np.float64)
    a = synth.make_jobs(rng, width, height, n_jobs, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=bipred)
    b = edge_jobs(rng, width, height, n_edge)
    jobs = np.concatenate([b[:8], a, b[8:]])
    # recompute the bi-pred keys over the final order
    jobs["key_offset"][(jobs["flags"] & JOB_BIPRED) != 0] = -2
    keys = synth.make_bipred_keys(rng, jobs, pics)
    ref = Reference(use_hadamard=hadme, nn_mode=nn_mode, fast_inter_mode=fen, bit_depth=bit_depth)
    orc = Oracle(use_hadamard=hadme, nn_mode=nn_mode, qp=qp, fast_inter_mode=fen, bit_depth=bit_depth)
    wts = weights.load_weights(qp)
    for eng in (ref, orc):
        for k, v in pics.items():
            eng.set_picture(k, v)
        for lid, lam in enumerate(lambdas):
            eng.set_lambda(lid, float(lam))
        eng.set_keys(keys if keys.size else np.zeros(1, np.int16))
        eng.load_nn(wts)
        if net is not None:
            eng.load_nn_net(weights.case_net(net))
    r_ref = ref.refine(jobs)
    r_orc = orc.refine(jobs)
    bad, first, counts = compare_results(r_ref, r_orc)
    if bad:
        raise SystemExit(f"{name}: oracle disagrees with _ref on {bad} jobs (first {first}): {counts}")
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(
        path,
        pictures=np.stack([pics[i] for i in range(5)]),
        lambdas=lambdas,
        keys=keys,
        jobs=jobs,
        results=r_ref,
        config=np.array([hadme, fen, nn_mode, qp], dtype=np.int32),
        **({"net": np.array(net)} if net is not None else {}),
        **({"bit_depth": np.array([bit_depth], np.int32)} if bit_depth != 8 else {}),
    )
    print(f"{path}: {len(jobs)} jobs, {int((jobs['flags'] & JOB_BIPRED != 0).sum())} bi-pred, "
          f"{int((r_ref['n_emi'] < 8).sum())} with < 8 EMI pushes")


def mc10_pictures(width, height, refs, seed):
    """Reference pictures at bit depth 10: synthetic 10-bit luma, chroma from the 8-bit generator
    with random low bits (every sample value 0..1023 reachable)."""
    rng = np.random.default_rng(seed + 1000)
    pics = {}
    for k in range(refs):
        cb, cr = synth.synth_chroma(width, height, k, seed=seed)
        lo = rng.integers(0, 4, size=(2,) + cb.shape, dtype=np.uint16)
        pics[k] = (synth.synth_luma_hbd(width, height, k, bit_depth=10, seed=seed),
                   (cb.astype(np.uint16) << 2) | lo[0], (cr.astype(np.uint16) << 2) | lo[1])
    return pics


def build_mc10_case(name, seed, width, height, bi_frac, mv_amp, identical_frac, fill=0):
    """Motion compensation at bit depth 10 (cfg *_main10.cfg InternalBitDepth 10): the predicted
    uint16 planes from _ref's TComInterpolationFilter / TComYuv::addAvg at bitDepth 10 (the C
    restatement's orc_mc is 8-bit: these fixtures pin the HIP path on the reference alone)."""
    rng = np.random.default_rng(seed)
    pics = mc10_pictures(width, height, 3, seed)
    jobs = synth.make_mc_partition(rng, width, height, [0, 1, 2], bi_frac=bi_frac, mv_amp=mv_amp,
                                   identical_frac=identical_frac)
    ref = Reference(bit_depth=10)
    for k, (y, cb, cr) in pics.items():
        ref.set_picture_yuv(k, y, cb, cr)
    y = np.full((height, width), fill, np.uint16)
    cb = np.full((height // 2, width // 2), fill, np.uint16)
    cr = cb.copy()
    ref.mc(jobs, y, cb, cr)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(
        path,
        ref_y=np.stack([pics[k][0] for k in range(3)]),
        ref_cb=np.stack([pics[k][1] for k in range(3)]),
        ref_cr=np.stack([pics[k][2] for k in range(3)]),
        jobs=jobs,
        fill=np.array([fill], np.uint16),
        bit_depth=np.array([10], np.int32),
        pred_y=y, pred_cb=cb, pred_cr=cr,
    )
    print(f"{path}: {len(jobs)} PUs, {int(((jobs['flags'] & 3) == 3).sum())} bi-pred, "
          f"luma {int(y.min())}..{int(y.max())}")


def wp_table(rng, refs):
    """Explicit WP parameters [list][ref][Y, Cb, Cr][iWeight, iOffset, uiLog2WeightDenom] as a slice
    header carries them: one luma and one chroma denominator per slice (0..7), weights
    2^denom + delta (delta -24..24, some exactly 2^denom to reach addWeightUni's unit-weight branch),
    offsets -128..127 (8-bit units) with some zero."""
    t = np.zeros((2, refs, 3, 3), np.int32)
    dl, dc = int(rng.integers(0, 8)), int(rng.integers(0, 8))
    for l in range(2):
        for r in range(refs):
            for c in range(3):
                d = dl if c == 0 else dc
                delta = 0 if rng.random() < 0.25 else int(rng.integers(-24, 25))
                off = 0 if rng.random() < 0.3 else int(rng.integers(-128, 128))
                t[l, r, c] = ((1 << d) + delta, off, d)
    return t


def build_mcwp_case(name, seed, width, height, bi_frac, mv_amp, identical_frac, wp_frac, bit_depth=8):
    """Motion compensation with explicit weighted prediction (FME_MC_WP; PPS UseWP / WPBiPred,
    TComPrediction.cpp:509-512, 612-619): the planes from _ref, which filters each list to the 14-bit
    values and runs the reference's own TComWeightPrediction::addWeightUni / addWeightBi
    (TComWeightPrediction.cpp:78-245) with getWpScaling's derivation; a share of the jobs without
    the flag (plain averaging) and identical bi motion kept as two lists under WP.  The C oracle's
    orc_mc_wp agrees at 8 bits (tests/test_mc_wp.py); the 10-bit fixture rests on the reference."""
    from nnfme.abi import MC_WP
    rng = np.random.default_rng(seed)
    if bit_depth > 8:
        pics = mc10_pictures(width, height, 3, seed)
    else:
        pics = {}
        for k in range(3):
            cb, cr = synth.synth_chroma(width, height, k, seed=seed)
            pics[k] = (synth.synth_luma(width, height, k, seed=seed), cb, cr)
    jobs = synth.make_mc_partition(rng, width, height, [0, 1, 2], bi_frac=bi_frac, mv_amp=mv_amp,
                                   identical_frac=identical_frac)
    wpm = rng.random(len(jobs)) < wp_frac
    jobs["flags"] = np.where(wpm, jobs["flags"] | MC_WP, jobs["flags"])
    wp = wp_table(rng, 3)
    ref = Reference(bit_depth=bit_depth)
    for k, (y, cb, cr) in pics.items():
        ref.set_picture_yuv(k, y, cb, cr)
    for l in range(2):
        for r in range(3):
            ref.set_wp(l, r, wp[l, r])
    dt = np.uint16 if bit_depth > 8 else np.uint8
    y = np.zeros((height, width), dt)
    cb = np.zeros((height // 2, width // 2), dt)
    cr = cb.copy()
    ref.mc(jobs, y, cb, cr)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(
        path,
        ref_y=np.stack([pics[k][0] for k in range(3)]),
        ref_cb=np.stack([pics[k][1] for k in range(3)]),
        ref_cr=np.stack([pics[k][2] for k in range(3)]),
        jobs=jobs, wp=wp, bit_depth=np.array([bit_depth], np.int32),
        pred_y=y, pred_cb=cb, pred_cr=cr,
    )
    bi = (jobs["flags"] & 3) == 3
    same = bi & (jobs["ref_id"][:, 0] == jobs["ref_id"][:, 1]) & (jobs["mv"][:, 0, 0] == jobs["mv"][:, 1, 0]) & \
        (jobs["mv"][:, 0, 1] == jobs["mv"][:, 1, 1])
    print(f"{path}: {len(jobs)} PUs, {int(wpm.sum())} weighted, {int((bi & wpm).sum())} weighted bi-pred, "
          f"{int((same & wpm).sum())} weighted identical-motion, denominators {int(wp[0, 0, 0, 2])}/{int(wp[0, 0, 1, 2])}")


MCWP_CASES = [
    # name, seed, W, H, bi fraction, MV amplitude, identical-motion fraction, WP fraction, bit depth
    ("mcwp_p_uni", 61, 160, 104, 0.0, 40, 0.0, 0.9, 8),
    ("mcwp_b_bi", 62, 168, 96, 0.6, 120, 0.2, 0.8, 8),
    ("mcwp10_b_bi", 63, 128, 80, 0.6, 60, 0.2, 0.8, 10),
]


def build_mc_case(name, seed, width, height, bi_frac, mv_amp, identical_frac, keep_frac=1.0, fill=0):
    """Motion compensation (TComPrediction::motionCompensation): reference pictures with 4:2:0
    chroma, one frame partition of decided PUs, the predicted planes from _ref (the oracle must
    agree).  keep_frac < 1 drops PUs: their samples must keep the initial `fill`."""
    from nnfme.abi import MC_JOB_DTYPE  # noqa: F401
    rng = np.random.default_rng(seed)
    pics = {}
    for k in range(3):
        cb, cr = synth.synth_chroma(width, height, k, seed=seed)
        pics[k] = (synth.synth_luma(width, height, k, seed=seed), cb, cr)
    if name == "mc_shapes":   # every HEVC inter PU shape once, each in its own 64x64 cell
        shapes = synth.ALL_PU_SIZES
        jobs = synth.make_mc_partition(rng, 64 * 6, 64 * 4, [0, 1, 2], bi_frac=bi_frac, mv_amp=mv_amp)[:len(shapes)]
        for i, (w, h) in enumerate(shapes):
            jobs[i]["x"], jobs[i]["y"] = 64 * (i % 6) + (64 - w), 64 * (i // 6)
            jobs[i]["cu_x"], jobs[i]["cu_y"] = 64 * (i % 6), 64 * (i // 6)
            jobs[i]["w"], jobs[i]["h"] = w, h
    else:
        jobs = synth.make_mc_partition(rng, width, height, [0, 1, 2], bi_frac=bi_frac, mv_amp=mv_amp,
                                       identical_frac=identical_frac)
    if keep_frac < 1.0:
        jobs = jobs[rng.random(len(jobs)) < keep_frac]
    ref, orc = Reference(), Oracle()
    for k, (y, cb, cr) in pics.items():
        ref.set_picture_yuv(k, y, cb, cr)
    outs = []
    for eng in (ref, orc):
        y = np.full((height, width), fill, np.uint8)
        cb = np.full((height // 2, width // 2), fill, np.uint8)
        cr = cb.copy()
        if eng is ref:
            eng.mc(jobs, y, cb, cr)
        else:
            eng.mc(pics, jobs, y, cb, cr)
        outs.append((y, cb, cr))
    for a, b, comp in zip(outs[0], outs[1], "Y Cb Cr".split()):
        if not np.array_equal(a, b):
            raise SystemExit(f"{name}: oracle disagrees with _ref on {comp} ({int((a != b).sum())} samples)")
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(
        path,
        ref_y=np.stack([pics[k][0] for k in range(3)]),
        ref_cb=np.stack([pics[k][1] for k in range(3)]),
        ref_cr=np.stack([pics[k][2] for k in range(3)]),
        jobs=jobs,
        fill=np.array([fill], np.uint8),
        pred_y=outs[0][0], pred_cb=outs[0][1], pred_cr=outs[0][2],
    )
    nbi = int(((jobs["flags"] & 3) == 3).sum())
    print(f"{path}: {len(jobs)} PUs, {nbi} bi-pred, {len(set(zip(jobs['w'], jobs['h'])))} PU shapes")


def tz_pictures(width, height, seed, bit_depth):
    """The integer-search fixtures' five pictures: 8-bit, or the same field at bit depth 10 (main10)."""
    if bit_depth > 8:
        return {i: synth.synth_luma_hbd(width, height, i, bit_depth=bit_depth, seed=seed) for i in range(5)}
    return {i: synth.synth_luma(width, height, i, seed=seed) for i in range(5)}


def build_tz_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, bit_depth=8):
    """Integer motion estimation (xTZSearch / xPatternSearch) from _ref; the oracle must agree.
    bit_depth 10: 16-bit pictures, the distortions of TComRdCost at bitDepth 10 (SSE (d * d) >> 4 per
    sample, SAD >> 2 per block)."""
    rng = np.random.default_rng(seed)
    pics = tz_pictures(width, height, seed, bit_depth)
    lambdas = np.array(synth.LDP_LAMBDA[22], dtype=np.float64)
    jobs, ext = synth.make_tz_jobs(rng, width, height, calls, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=bipred,
                                   search_range=search_range, mvp_noise=mvp_noise)
    keys = synth.make_bipred_keys(rng, jobs, pics)
    ref = Reference(fast_inter_mode=fen, bit_depth=bit_depth)
    orc = Oracle(fast_inter_mode=fen, bit_depth=bit_depth)
    for eng in (ref, orc):
        for k, v in pics.items():
            eng.set_picture(k, v)
        for lid, lam in enumerate(lambdas):
            eng.set_lambda(lid, float(lam))
        eng.set_keys(keys if keys.size else np.zeros(1, np.int16))
    out_r, sad_r = ref.integer_search(jobs, ext)
    out_o, sad_o = orc.integer_search(jobs, ext)
    bad = (out_r["mv_x"] != out_o["mv_x"]) | (out_r["mv_y"] != out_o["mv_y"]) | (sad_r != sad_o)
    if bad.any():
        raise SystemExit(f"{name}: oracle disagrees with _ref on {int(bad.sum())} jobs")
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, pictures=np.stack([pics[i] for i in range(5)]), lambdas=lambdas, keys=keys,
                        jobs=jobs, ext=ext, mv_x=out_r["mv_x"], mv_y=out_r["mv_y"], sad=sad_r,
                        config=np.array([fen, search_range], dtype=np.int32),
                        **({"bit_depth": np.array([bit_depth], np.int32)} if bit_depth != 8 else {}))
    far = np.abs(out_r["mv_x"] * 4 - jobs["mvp_x"]) + np.abs(out_r["mv_y"] * 4 - jobs["mvp_y"])
    print(f"{path}: {len(jobs)} jobs, {int((jobs['flags'] & JOB_BIPRED != 0).sum())} bi-pred, "
          f"{int((ext['flags'] != 0).sum())} with a 2Nx2N start, {int((far > 4 * 20).sum())} ending > 20 px from the predictor")


def build_tz2_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, mode, bit_depth=8):
    """The other FastSearch settings (fme_tz_ext2): FastSearch 0 (FME_TZ_FULL, xPatternSearch for every
    job) or 3 (FME_TZ_ENHANCED, xTZSearch with bExtendedSettings and the neighbour predictors
    m_acMvPredictors) from _ref; the oracle must agree.  The predictors: near the AMVP predictor, some
    equal to it, some zero, some far (the start-point tests' "not obviously previously tested"
    conditions both ways)."""
    from nnfme.abi import TZ_EXT2_DTYPE
    rng = np.random.default_rng(seed)
    pics = tz_pictures(width, height, seed, bit_depth)
    lambdas = np.array(synth.LDP_LAMBDA[22], dtype=np.float64)
    jobs, ext = synth.make_tz_jobs(rng, width, height, calls, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=bipred,
                                   search_range=search_range, mvp_noise=mvp_noise)
    keys = synth.make_bipred_keys(rng, jobs, pics)
    n = len(jobs)
    ext2 = np.zeros(n, dtype=TZ_EXT2_DTYPE)
    ext2["base"] = ext
    uni = (jobs["flags"] & JOB_BIPRED) == 0
    ext2["base"]["flags"] = np.where(uni, ext["flags"] | mode, ext["flags"])
    kind = rng.integers(0, 4, (n, 3))
    for c, comp in ((0, "mvp_x"), (1, "mvp_y")):
        base = jobs[comp].astype(np.int64)[:, None]
        near = base + rng.integers(-12, 13, (n, 3))
        far = rng.integers(-4 * 3 * search_range, 4 * 3 * search_range + 1, (n, 3))
        v = np.where(kind == 0, base, np.where(kind == 1, 0, np.where(kind == 2, near, far)))
        ext2["preds"][:, :, c] = np.clip(v, -32768, 32767)
    ref = Reference(fast_inter_mode=fen, bit_depth=bit_depth)
    orc = Oracle(fast_inter_mode=fen, bit_depth=bit_depth)
    for eng in (ref, orc):
        for k, v in pics.items():
            eng.set_picture(k, v)
        for lid, lam in enumerate(lambdas):
            eng.set_lambda(lid, float(lam))
        eng.set_keys(keys if keys.size else np.zeros(1, np.int16))
    out_r, sad_r = ref.integer_search2(jobs, ext2)
    out_o, sad_o = orc.integer_search2(jobs, ext2)
    bad = (out_r["mv_x"] != out_o["mv_x"]) | (out_r["mv_y"] != out_o["mv_y"]) | (sad_r != sad_o)
    if bad.any():
        raise SystemExit(f"{name}: oracle disagrees with _ref on {int(bad.sum())} jobs")
    # against the shipped FastSearch 1 on the same jobs: the setting changes results
    base_r, _ = ref.integer_search(jobs, ext)
    differ = int(((base_r["mv_x"] != out_r["mv_x"]) | (base_r["mv_y"] != out_r["mv_y"])).sum())
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, pictures=np.stack([pics[i] for i in range(5)]), lambdas=lambdas, keys=keys,
                        jobs=jobs, ext=ext2, mv_x=out_r["mv_x"], mv_y=out_r["mv_y"], sad=sad_r,
                        config=np.array([fen, search_range], dtype=np.int32),
                        **({"bit_depth": np.array([bit_depth], np.int32)} if bit_depth != 8 else {}))
    print(f"{path}: {n} jobs, {int((~uni).sum())} bi-pred, mode 0x{mode:x}, {differ} MVs differ from FastSearch 1")


def build_ring_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, net, qp=22):
    """The backups' own NN input path (configs[4]): xTZSearch with the final square + ring, every
    distortion pushed (FME_TZ_RING: mv, sad and the nine NN inputs per job), then the sub-pel path
    with the deeper net on those inputs (FME_JOB_NN_IN; bi-pred jobs reuse the last uni-pred call's
    inputs).  Both stages from _ref; the oracle must agree on every output."""
    rng = np.random.default_rng(seed)
    pics = {i: synth.synth_luma(width, height, i, seed=seed) for i in range(5)}
    lambdas = np.array(synth.LDP_LAMBDA[qp], dtype=np.float64)
    jobs, ext = synth.make_tz_jobs(rng, width, height, calls, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=bipred,
                                   search_range=search_range, mvp_noise=mvp_noise)
    ext["flags"] |= TZ_RING
    keys = synth.make_bipred_keys(rng, jobs, pics)
    ref = Reference(use_hadamard=1, nn_mode=2, fast_inter_mode=fen)
    orc = Oracle(use_hadamard=1, nn_mode=2, qp=qp, fast_inter_mode=fen)
    nnet = weights.case_net(net)
    for eng in (ref, orc):
        for k, v in pics.items():
            eng.set_picture(k, v)
        for lid, lam in enumerate(lambdas):
            eng.set_lambda(lid, float(lam))
        eng.set_keys(keys if keys.size else np.zeros(1, np.int16))
        eng.load_nn_net(nnet)
    out_r, sad_r, nn_r = ref.integer_search_ring(jobs, ext)
    out_o, sad_o, nn_o = orc.integer_search_ring(jobs, ext)
    bad = (out_r["mv_x"] != out_o["mv_x"]) | (out_r["mv_y"] != out_o["mv_y"]) | (sad_r != sad_o) | \
        (nn_r != nn_o).any(axis=1)
    if bad.any():
        raise SystemExit(f"{name}: oracle disagrees with _ref's integer search on {int(bad.sum())} jobs")
    uni = (jobs["flags"] & JOB_BIPRED) == 0
    rjobs = out_r.copy()
    rjobs["flags"] = np.where(uni, JOB_NN_IN, rjobs["flags"]).astype(np.uint8)
    for eng in (ref, orc):
        eng.set_nn_inputs(nn_r)
    r_ref = ref.refine(rjobs)
    r_orc = orc.refine(rjobs)
    bad, first, counts = compare_results(r_ref, r_orc)
    if bad:
        raise SystemExit(f"{name}: oracle disagrees with _ref on {bad} refinements (first {first}): {counts}")
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, pictures=np.stack([pics[i] for i in range(5)]), lambdas=lambdas, keys=keys,
                        jobs=jobs, ext=ext, mv_x=out_r["mv_x"], mv_y=out_r["mv_y"], sad=sad_r, nn_in=nn_r,
                        refine_jobs=rjobs, results=r_ref, net=np.array(net),
                        config=np.array([1, fen, 2, qp, search_range], dtype=np.int32))
    moved = ((out_r["mv_x"] != orc.integer_search(jobs, ext)[0]["mv_x"]) & uni).sum()
    print(f"{path}: {len(jobs)} jobs, {int((~uni).sum())} bi-pred, {int(moved)} moved by the square + ring, "
          f"{int((nn_r[uni, :8] == 0).any(axis=1).sum())} with < 8 pushes, classes {len(set(r_ref['nn_class']))}")


RING_CASES = [
    # name, seed, W, H, calls/CTU/ref, FEN, SearchRange, bi-pred share, predictor noise, net
    ("ring_scr3x40_fen1", 41, 160, 96, 40, 1, 64, 0.15, 24, "scr3x40+tzring"),
    ("ring_b4x40_sr8_fen3", 42, 128, 96, 40, 3, 8, 0.1, 60, "blowing4x40+rezero+tzring"),
    # SearchRange 2: the square and the ring mostly clipped by the range (fewer than 8 pushes)
    ("ring_scr3x40_sr2_fen0", 43, 128, 96, 30, 0, 2, 0.1, 24, "scr3x40+tzring"),
]

TZ_CASES = [
    # name, seed, W, H, calls/CTU/ref, FEN, SearchRange, bi-pred share, predictor noise (qpel)
    ("tz_ldp_fen1", 31, 160, 96, 40, 1, 64, 0.15, 24),
    ("tz_far_fen0_sr32", 32, 160, 96, 40, 0, 32, 0.1, 200),
]

TZ2_CASES = [
    # name, seed, W, H, calls/CTU/ref, FEN, SearchRange, bi-pred share, predictor noise (qpel), mode
    ("tz_full_sr8_fen1", 33, 128, 96, 10, 1, 8, 0.1, 24, 0x04),
    ("tz_enhanced_fen1", 34, 160, 96, 30, 1, 64, 0.1, 24, 0x08),
    ("tz_enhanced_far_fen0_sr32", 35, 160, 96, 30, 0, 32, 0.1, 200, 0x08),
]

TZ10_CASES = [
    # bit depth 10 (the main10 configurations): FastSearch 1 / 0 / 3 with SSE and the SAD widths
    # (FEN 0 and the FEN 1 / 3 row subsampling); (TZ_CASES fields, mode or None, bit depth)
    ("tz10_ldp_fen1", 51, 160, 96, 40, 1, 64, 0.15, 24, None, 10),
    ("tz10_far_fen0_sr32", 52, 160, 96, 40, 0, 32, 0.1, 200, None, 10),
    ("tz10_full_sr8_fen3", 53, 128, 96, 10, 3, 8, 0.1, 24, 0x04, 10),
    ("tz10_enhanced_fen1", 54, 160, 96, 30, 1, 64, 0.1, 24, 0x08, 10),
]


def build_tz10_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, mode, bit_depth):
    if mode is None:
        build_tz_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, bit_depth=bit_depth)
    else:
        build_tz2_case(name, seed, width, height, calls, fen, search_range, bipred, mvp_noise, mode,
                       bit_depth=bit_depth)


MC10_CASES = [
    # name, seed, W, H, bi fraction, MV amplitude (quarter-pel), identical-motion fraction, fill
    ("mc10_ldp_uni", 41, 160, 104, 0.0, 40, 0.0, 0),
    ("mc10_ra_bi_clip", 42, 168, 96, 0.5, 200, 0.2, 0),
    ("mc10_bi_near", 43, 128, 80, 0.8, 12, 0.1, 513),
]

MC_CASES = [
    # name, seed, W, H, bi_frac, mv_amp (pel), identical_frac, keep_frac, fill
    ("mc_ldp_uni", 21, 160, 104, 0.0, 40, 0.0, 1.0, 0),
    ("mc_ra_bi_clip", 22, 168, 96, 0.5, 200, 0.2, 1.0, 0),
    ("mc_sparse", 23, 128, 80, 0.3, 16, 0.1, 0.5, 77),
    ("mc_shapes", 24, 384, 256, 0.5, 24, 0.0, 1.0, 9),
]

CASES = [
    # name, seed, W, H, jobs, HADME, FEN, nn_mode, QP
    ("ldp_qp22_hadme_fen1_nn", 11, 160, 96, 1200, 1, 1, 1, 22),
    ("sad_fen0_nnoff", 12, 160, 96, 600, 0, 0, 0, 22),
    ("fen3_qp27_nn", 13, 128, 96, 400, 1, 3, 1, 27),
    ("qp32_nn", 14, 128, 96, 400, 1, 1, 1, 32),
    ("qp37_nn", 15, 128, 96, 400, 1, 1, 1, 37),
    # configs[1] exactly: HADME on, FEN 1, NN_pred off (the standard FracDIF MV)
    ("hadme_fen1_nnoff_qp22", 18, 160, 96, 800, 1, 1, 0, 22),
    # configs[3]'s random-access lambdas (GOP-8 depths 0..3) with its bi-pred share
    ("ra_qp27_nn", 19, 160, 96, 800, 1, 1, 1, 27, 0.205, 96, None, "ra"),
]


# main10 (InternalBitDepth 10, cfg/encoder_lowdelay_P_main10.cfg:58 and the RA / LD main10 cfgs):
# the sub-pel path with 16-bit pictures; every PU shape, edges, lossless jobs, bi-pred keys
MAIN10_CASES = [
    # name, seed, W, H, jobs, HADME, FEN, nn_mode, QP, bi-pred, edge jobs, net, gop, bit depth
    ("main10_ldp_qp22_hadme_fen1_nn", 51, 160, 96, 1200, 1, 1, 1, 22, 0.15, 96, None, "ldp", 10),
    ("main10_sad_fen0_nnoff", 52, 160, 96, 600, 0, 0, 0, 22, 0.15, 96, None, "ldp", 10),
    ("main10_fen3_qp27_nn", 53, 128, 96, 500, 1, 3, 1, 27, 0.15, 96, None, "ldp", 10),
    ("main10_ra_qp37_nn", 54, 128, 96, 500, 1, 1, 1, 37, 0.205, 96, None, "ra", 10),
]


# nn_mode 2: the reference's deeper nets (BASELINE.json configs[4]) and the master net through the
# generic path.  nn4x40 runs with its X3/X4 carry cleared ("+rezero"): the batch engines do not run
# carried hidden layers (fme_load_nn_net rejects carry_hidden); the oracle and _ref cover both.
DEEP_CASES = [
    ("deep_scr3x40_qp22", 16, 160, 96, 900, 1, 1, 2, 22, 0.15, 96, "scr3x40"),
    ("deep_blowing4x40_qp22", 17, 128, 96, 600, 1, 1, 2, 22, 0.15, 96, "blowing4x40+rezero"),
    ("deep_master_qp22", 11, 160, 96, 1200, 1, 1, 2, 22, 0.15, 96, "master"),
]


# ---- stress content (tests/golden/stress/): saturated, flat and two-level pictures ---------------------
# In a subdirectory: tests/conftest.py's golden_cases() takes every top-level .npz as a refinement case.
STRESS_OUT = os.path.join(OUT, "stress")
STRESS_W, STRESS_H, STRESS_MC_H = 128, 128, 64
STRESS_LAMBDAS = synth.LDP_LAMBDA[22] + (0.0,)   # slot 4: lambda 0 (the integer search's jobs use it)
STRESS_REFINE_SETS = ("checker1", "binary", "flat", "twolevel", "full-zero")
STRESS_TZ_SETS = (("binary", 8), ("checker1", 8), ("flat", 8), ("flat", 32))   # (set, SearchRange)
STRESS_MC_KINDS = ("binary", "checker1", "full")
STRESS_KEY_SETS = ("full-zero", "zero-full", "binary")
STRESS_TEMPLATE_SETS = ("flat", "twolevel", "binary", "checker1")


def stress_seeded(name):
    """Whether a stress set (KIND or ORG-REF) holds a seeded kind: only those planes are stored."""
    return any(k in synth.STRESS_SEEDED for k in name.split("-"))


def save_stress(name, arrays):
    """An .npz whose bytes depend on the arrays alone (numpy's own writer stamps the time)."""
    import io
    import zipfile
    os.makedirs(STRESS_OUT, exist_ok=True)
    path = os.path.join(STRESS_OUT, name + ".npz")
    with zipfile.ZipFile(path, "w") as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


def _stress_engines(pics, keys, bit_depth, **cfg):
    """(Reference, Oracle) on the same pictures, STRESS_LAMBDAS and keys."""
    ocfg = dict(cfg)
    if "nn_mode" in cfg:
        ocfg["qp"] = 22
    ref, orc = Reference(bit_depth=bit_depth, **cfg), Oracle(bit_depth=bit_depth, **ocfg)
    for eng in (ref, orc):
        for k, v in pics.items():
            eng.set_picture(k, v)
        for lid, lam in enumerate(STRESS_LAMBDAS):
            eng.set_lambda(lid, float(lam))
        if keys is not None:
            eng.set_keys(keys if keys.size else np.zeros(1, np.int16))
        if cfg.get("nn_mode"):
            eng.load_nn(weights.load_weights(22))
    return ref, orc


def build_stress_refine(bit_depth):
    """refine: per stress set one batch (synth.stress_refine_batch), HADME 1 and 0, NN on."""
    out = {"sets": np.array(STRESS_REFINE_SETS), "lambdas": np.array(STRESS_LAMBDAS)}
    for si, name in enumerate(STRESS_REFINE_SETS):
        pics = synth.stress_pictures(STRESS_W, STRESS_H, bit_depth, name)
        # (seed base 704: on `flat` every job then has a tied half and quarter stage at both depths; a
        # predictor within 2 quarter-pels of the start on both axes makes the centre the only minimum)
        jobs, keys = synth.stress_refine_batch(np.random.default_rng(704 + 10 * bit_depth + si), STRESS_W, STRESS_H,
                                               bit_depth, pics)
        out[f"{name}.jobs"], out[f"{name}.keys"] = jobs, keys
        if stress_seeded(name):
            out[f"{name}.pictures"] = np.stack([pics[k] for k in range(5)])
        for hadme in (1, 0):
            ref, orc = _stress_engines(pics, keys, bit_depth, use_hadamard=hadme, nn_mode=1, fast_inter_mode=1)
            r_ref, r_orc = ref.refine(jobs), orc.refine(jobs)
            bad, first, counts = compare_results(r_ref, r_orc)
            if bad:
                raise SystemExit(f"stress refine {name} {bit_depth} bits HADME {hadme}: oracle disagrees with _ref "
                                 f"on {bad} jobs (first {first}): {counts}")
            out[f"{name}.results_hadme{hadme}"] = r_ref
    save_stress(f"refine{bit_depth}", out)


def build_stress_tz(bit_depth):
    """integer_search: per (stress set, SearchRange) one batch (synth.stress_tz_batch), FEN 0 / 1 / 3."""
    out = {"sets": np.array([f"{n}.sr{sr}" for n, sr in STRESS_TZ_SETS]), "lambdas": np.array(STRESS_LAMBDAS)}
    for si, (name, sr) in enumerate(STRESS_TZ_SETS):
        pics = synth.stress_pictures(STRESS_W, STRESS_H, bit_depth, name)
        jobs, ext, keys = synth.stress_tz_batch(np.random.default_rng(800 + 10 * bit_depth + si), STRESS_W, STRESS_H,
                                                bit_depth, pics, search_range=sr)
        case = f"{name}.sr{sr}"
        out[f"{case}.jobs"], out[f"{case}.ext"], out[f"{case}.keys"] = jobs, ext, keys
        if stress_seeded(name):
            out[f"{case}.pictures"] = np.stack([pics[k] for k in range(5)])
        for fen in (0, 1, 3):
            ref, orc = _stress_engines(pics, keys, bit_depth, fast_inter_mode=fen)
            out_r, sad_r = ref.integer_search(jobs, ext)
            out_o, sad_o = orc.integer_search(jobs, ext)
            bad = (out_r["mv_x"] != out_o["mv_x"]) | (out_r["mv_y"] != out_o["mv_y"]) | (sad_r != sad_o)
            if bad.any():
                raise SystemExit(f"stress tz {case} {bit_depth} bits FEN {fen}: oracle disagrees with _ref on "
                                 f"{int(bad.sum())} jobs")
            out[f"{case}.mv_fen{fen}"] = np.stack([out_r["mv_x"], out_r["mv_y"]], axis=1)
            out[f"{case}.sad_fen{fen}"] = sad_r
    save_stress(f"tz{bit_depth}", out)


def stress_wp_table(rng, refs):
    """wp_table's extremes: denominators 0 and 7, weights 2^denom - 24 / + 24 / + 0, offsets -128 / 127 / 0."""
    t = np.zeros((2, refs, 3, 3), np.int32)
    dl = int(rng.integers(0, 2)) * 7
    for l in range(2):
        for r in range(refs):
            for c in range(3):
                d = dl if c == 0 else 7 - dl
                t[l, r, c] = ((1 << d) + (-24, 24, 0)[int(rng.integers(0, 3))], (-128, 127, 0)[int(rng.integers(0, 3))], d)
    return t


def build_stress_mc(bit_depth):
    """mc: 128x64 4:2:0 references of each kind; uni, bi and explicit WP at wp_table's extremes, MVs
    out to +-600 quarter-pels (clipMv bites).  The oracle checks all but the 10-bit WP case."""
    from nnfme.abi import MC_WP
    W, H = STRESS_W, STRESS_MC_H
    dt = np.uint16 if bit_depth > 8 else np.uint8
    out = {"kinds": np.array(STRESS_MC_KINDS), "modes": np.array(["uni", "bi", "wp"])}
    for ki, kind in enumerate(STRESS_MC_KINDS):
        pics = synth.stress_yuv(W, H, bit_depth, kind)
        if stress_seeded(kind):
            for c, comp in enumerate(("y", "cb", "cr")):
                out[f"{kind}.ref_{comp}"] = np.stack([pics[k][c] for k in range(3)])
        for mi, (mode, bi_frac) in enumerate((("uni", 0.0), ("bi", 0.7), ("wp", 0.5))):
            rng = np.random.default_rng(900 + 100 * bit_depth + 10 * ki + mi)
            # every CTU split at least once: 128x64 holds two, and two 64x64 PUs would be the whole case
            jobs = synth.make_mc_partition(rng, W, H, [0, 1, 2], bi_frac=bi_frac, mv_amp=150, identical_frac=0.1,
                                           p_split=(1.0, 0.7, 0.5))
            wp = None
            if mode == "wp":
                jobs["flags"] = np.where(rng.random(len(jobs)) < 0.8, jobs["flags"] | MC_WP, jobs["flags"])
                wp = stress_wp_table(rng, 3)
            ref, orc = Reference(bit_depth=bit_depth), Oracle(bit_depth=bit_depth)
            for k, v in pics.items():
                ref.set_picture_yuv(k, *v)
            if wp is not None:
                for l in range(2):
                    for r in range(3):
                        ref.set_wp(l, r, wp[l, r])
            planes = [[np.zeros((H, W), dt), np.zeros((H // 2, W // 2), dt), np.zeros((H // 2, W // 2), dt)]
                      for _ in range(2)]
            ref.mc(jobs, *planes[0])
            if wp is None or bit_depth == 8:
                orc.mc(pics, jobs, *planes[1], wp=wp)
                for a, b, comp in zip(planes[0], planes[1], "Y Cb Cr".split()):
                    if not np.array_equal(a, b):
                        raise SystemExit(f"stress mc {kind} {mode} {bit_depth} bits: oracle disagrees with _ref on "
                                         f"{comp} ({int((a != b).sum())} samples)")
            case = f"{kind}.{mode}"
            out[f"{case}.jobs"] = jobs
            if wp is not None:
                out[f"{case}.wp"] = wp
            for p, comp in zip(planes[0], ("y", "cb", "cr")):
                out[f"{case}.pred_{comp}"] = p
    save_stress(f"mc{bit_depth}", out)


def build_stress_bi_key(bit_depth):
    """bi_key: every PU shape twice, all bi-pred, the other list's MV out to +-200 quarter-pels, with
    and without ClipForBiPredMeEnabled; full against zero and the reverse reach both ends."""
    out = {"sets": np.array(STRESS_KEY_SETS)}
    shapes = np.array(synth.ALL_PU_SIZES)
    for si, name in enumerate(STRESS_KEY_SETS):
        pics = synth.stress_pictures(STRESS_W, STRESS_H, bit_depth, name)
        rng = np.random.default_rng(1000 + 10 * bit_depth + si)
        jobs = synth.make_jobs(rng, STRESS_W, STRESS_H, 48, 4, [0, 1, 2, 3], [0, 1, 2, 3],
                               sizes=(np.tile(shapes[:, 0], 2), np.tile(shapes[:, 1], 2)))
        jobs["flags"] = JOB_BIPRED
        jobs["key_offset"] = -2
        reqs, count = synth.make_bipred_key_reqs(rng, jobs, 4, [0, 1, 2, 3], mv_span=200)
        out[f"{name}.jobs"], out[f"{name}.reqs"] = jobs, reqs
        if stress_seeded(name):
            out[f"{name}.pictures"] = np.stack([pics[k] for k in range(5)])
        ref, orc = _stress_engines(pics, None, bit_depth)
        for clip in (0, 1):
            keys = np.zeros(count, np.int16)
            for q in reqs:
                args = [int(q[f]) for f in ("org_id", "ref_id", "x", "y", "w", "h", "cu_x", "cu_y", "mv_x", "mv_y")]
                a, b = ref.bi_key(*args, clip), orc.bi_key(*args, clip)
                if not np.array_equal(a, b):
                    raise SystemExit(f"stress bi_key {name} {bit_depth} bits clip {clip}: oracle disagrees with _ref")
                keys[int(q["key_offset"]):int(q["key_offset"]) + a.size] = a.reshape(-1)
            out[f"{name}.keys_clip{clip}"] = keys
    save_stress(f"bikey{bit_depth}", out)


def stress_template_requests(rng, n, width, height):
    """CUs at every quadtree depth, every PU shape that fits, two candidates per reference, MVs near
    and far (clipMv active): tests/test_pred_inter.py's stream on a width x height picture."""
    from nnfme.abi import PU_REQ_DTYPE
    reqs = np.zeros(n, dtype=PU_REQ_DTYPE)
    for i in range(n):
        w, h = synth.ALL_PU_SIZES[i % len(synth.ALL_PU_SIZES)]
        cu = max(8, 1 << int(np.ceil(np.log2(max(w, h)))))
        cu_x, cu_y = cu * int(rng.integers(0, width // cu)), cu * int(rng.integers(0, height // cu))
        reqs[i]["x"] = cu_x + 4 * int(rng.integers(0, (cu - w) // 4 + 1))
        reqs[i]["y"] = cu_y + 4 * int(rng.integers(0, (cu - h) // 4 + 1))
        reqs[i]["w"], reqs[i]["h"], reqs[i]["cu_x"], reqs[i]["cu_y"] = w, h, cu_x, cu_y
        reqs[i]["depth"] = {64: 0, 32: 1, 16: 2, 8: 3}[cu]
        reqs[i]["org_id"], reqs[i]["num_refs"], reqs[i]["ref_id"] = 4, 4, [0, 1, 2, 3]
        reqs[i]["n_cand"] = [2, 2, 1, 2]
        span = 220 if rng.random() < 0.3 else 40
        reqs[i]["cand"] = rng.integers(-4 * span, 4 * span + 1, (4, 2, 2))
        reqs[i]["lambda_id"] = int(rng.integers(0, 4))
    return reqs


def build_stress_template(bit_depth):
    """template_cost: xGetTemplateCost per (request, reference, candidate) on 128x64 stress sets."""
    out = {"sets": np.array(STRESS_TEMPLATE_SETS)}
    for si, name in enumerate(STRESS_TEMPLATE_SETS):
        pics = synth.stress_pictures(STRESS_W, STRESS_MC_H, bit_depth, name)
        reqs = stress_template_requests(np.random.default_rng(1100 + 10 * bit_depth + si), 72, STRESS_W, STRESS_MC_H)
        ref, orc = _stress_engines(pics, None, bit_depth, fast_inter_mode=1)
        cost = np.full((len(reqs), 4, 2), 0xFFFFFFFF, np.uint32)
        for i, q in enumerate(reqs):
            for k in range(4):
                for m in range(int(q["n_cand"][k])):
                    mx, my = (int(v) for v in q["cand"][k][m])
                    cost[i, k, m] = ref.template_cost(4, int(q["ref_id"][k]), int(q["x"]), int(q["y"]), int(q["w"]),
                                                      int(q["h"]), int(q["cu_x"]), int(q["cu_y"]), mx, my, 1,
                                                      int(q["lambda_id"]))
                    if orc.template_cost(q, k, m) != cost[i, k, m]:
                        raise SystemExit(f"stress template_cost {name} {bit_depth} bits: oracle disagrees with _ref")
        out[f"{name}.reqs"], out[f"{name}.cost"] = reqs, cost
        if stress_seeded(name):
            out[f"{name}.pictures"] = np.stack([pics[k] for k in range(5)])
    save_stress(f"template{bit_depth}", out)


def build_stress():
    for bit_depth in (8, 10):
        build_stress_refine(bit_depth)
        build_stress_tz(bit_depth)
        build_stress_mc(bit_depth)
        build_stress_bi_key(bit_depth)
        build_stress_template(bit_depth)


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--stress-only" in sys.argv:
        build_stress()
        return 0
    only =sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    if only:
        for c in CASES + DEEP_CASES:
            if c[0] in only:
                build_case(*c)
        return 0
    if "--deep-only" in sys.argv:
        for c in DEEP_CASES:
            build_case(*c)
        return 0
    if "--main10-only" in sys.argv:
        for c in MAIN10_CASES:
            build_case(*c)
        return 0
    if "--tz2-only" in sys.argv:
        for c in TZ2_CASES:
            build_tz2_case(*c)
        return 0
    if "--tz10-only" in sys.argv:
        for c in TZ10_CASES:
            build_tz10_case(*c)
        return 0
    if "--mcwp-only" in sys.argv:
        for c in MCWP_CASES:
            build_mcwp_case(*c)
        return 0
    if "--mc10-only" in sys.argv:
        for c in MC10_CASES:
            build_mc10_case(*c)
        return 0
    if "--ring-only" in sys.argv:
        for c in RING_CASES:
            build_ring_case(*c)
        return 0
    for c in RING_CASES:
        build_ring_case(*c)
    for c in DEEP_CASES:
        build_case(*c)
    if "--mc-only" not in sys.argv and "--tz-only" not in sys.argv:
        for c in CASES + MAIN10_CASES:
            build_case(*c)
    if "--tz-only" not in sys.argv:
        for c in MC_CASES:
            build_mc_case(*c)
        for c in MC10_CASES:
            build_mc10_case(*c)
        for c in MCWP_CASES:
            build_mcwp_case(*c)
    for c in TZ_CASES:
        build_tz_case(*c)
    for c in TZ2_CASES:
        build_tz2_case(*c)
    for c in TZ10_CASES:
        build_tz10_case(*c)
    if "--mc-only" not in sys.argv and "--tz-only" not in sys.argv:
        build_stress()
    return 0


if __name__ == "__main__":
    sys.exit(main())
