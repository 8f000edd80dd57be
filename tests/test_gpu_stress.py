"""Saturated, flat and two-level pictures through every kernel (nnfme.synth.stress_picture; the keys
of bi-pred jobs at the ends of their range, synth.extreme_keys).

The sinusoid pictures of the other GPU tests keep every difference small and every tie rare.  Here
each batch kernel sees what its packed arithmetic and its parallel minima rest on: 0 / max transitions
(the filters' extreme outputs, the clip after the second stage, |d| = 2^b - 1), keys of -(2^b - 1) and
2 (2^b - 1) (|d| = 2046 at 10 bits, the bound of fme_lane10.hip's packed Hadamard; 64x64 sums near
2^32 in the integer search and the skip SSE), and flat or two-level pictures on which every candidate
of a stage ties, so that only the visiting order decides (the (cost, call index) minima of fme_tz.hip,
the lane kernels' per-lane decisions, the producers' first-strict-minimum choices).

Everything is bit-exact: against the fixtures of tests/golden/stress (oracle/_ref's results) where one
exists, and against the C oracle or the numpy mirrors, whose agreement with the oracle on this content
tests/test_stress_oracle.py checks on the CPU.  Pictures are 128x128 (128x64 for chroma and the
producers): two CTUs each way, so border windows and windows across tiles occur."""
import functools
import os

import numpy as np
import pytest

from nnfme import abi, merge, skip, surface, synth
from nnfme.abi import JOB_BIPRED, MC_JOB_DTYPE, MV_FIELDS, TZ_RING, compare_results
from test_gpu_lane_tiles import FIELDS
from test_stress_oracle import (DEPTHS, H, LAMBDAS, MC_H, REFINE_KINDS, W, case_pictures, hi_of, load_stress, mc_case,
                                mc_clip_bites, merge_case, oracle_for, pred_inter_b_case, pred_inter_p_case,
                                refine_case, refine_expected, setup, surface_jobs, tz_case)

pytestmark = pytest.mark.gpu

VARIANTS = ("d8", "d10", "d10px")   # bit depth 8; 10 with the default search; 10 with FME_MAIN10_SEARCH=px
SMALL_SETS = ("checker1", "binary", "full-zero", "flat")
PRODUCER_KINDS = ("flat", "twolevel", "binary", "checker1")


def _depth(variant):
    return 8 if variant == "d8" else 10


def _ctx(variant, **kw):
    """A context of the variant; FME_MAIN10_SEARCH is read once, when the context is created."""
    from nnfme.runtime import FmeContext
    old = os.environ.get("FME_MAIN10_SEARCH")
    if variant == "d10px":
        os.environ["FME_MAIN10_SEARCH"] = "px"
    else:
        os.environ.pop("FME_MAIN10_SEARCH", None)
    try:
        return FmeContext(bit_depth=_depth(variant), **kw)
    finally:
        if old is None:
            os.environ.pop("FME_MAIN10_SEARCH", None)
        else:
            os.environ["FME_MAIN10_SEARCH"] = old


def _same_records(got, want, what):
    bad, first, counts = compare_results(got, want, FIELDS)   # and emi: the n_emi pushed values
    assert bad == 0, f"{what}: {bad} of {len(got)} jobs differ, first {first}: {counts}"


# ---- refine: k_search_lane, k_search_lane10, fme_px.hip, the NN tail -------------------------------------
@pytest.mark.parametrize("hadme", [1, 0])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", REFINE_KINDS)
def test_refine(name, variant, hadme):
    """96 jobs: every PU shape uni-pred, on keys at the ends of the key range in every pattern, on
    ordinary keys, and lossless.  Every record field and the pushed EMI values against the fixture and
    the oracle, the NN state after the batch, and fme_refine_mv's records from a reset state."""
    bd = _depth(variant)
    pics, jobs, keys = refine_case(name, bd)
    want, state = refine_expected(name, bd, hadme)
    ctx = _ctx(variant, use_hadamard=hadme, nn_mode=1, qp=22, fast_inter_mode=1)
    try:
        setup(ctx, pics, keys)
        got = ctx.refine(jobs)
        assert ctx.refine_status() == 0
        after = ctx.nn_get_state()
        ctx.nn_reset()
        mv = ctx.refine_mv(jobs)
    finally:
        ctx.close()
    _same_records(got, want, f"{name} {variant} HADME {hadme} against the oracle")
    g = load_stress(f"refine{bd}")
    if name in g["sets"]:
        _same_records(got, g[f"{name}.results_hadme{hadme}"], f"{name} {variant} HADME {hadme} against the fixture")
    assert np.array_equal(after, state)
    for f in MV_FIELDS:
        assert np.array_equal(mv[f], want[f]), f"{name} {variant} HADME {hadme}: fme_mv_result.{f}"


def _single8_range_case(ref_plane):
    """tests/test_gpu_single10.py's _range_case at 8 bits: 64x64 and 8x4 bi-pred jobs against
    ref_plane, keys of -255 and 510 in 4x4 blocks, in 2x1 blocks, all 510 and all -255."""
    from test_gpu_parity import _frac_single_check
    pics = synth.stress_pictures(W, H, 8, "uniform")
    pics[0] = ref_plane
    rng = np.random.default_rng(104)
    w, h = np.array([64, 8, 64, 8, 64, 8]), np.array([64, 4, 64, 4, 64, 4])
    jobs = synth.make_jobs(rng, W, H, len(w), 4, [0], [0, 1, 2, 3], sizes=(w, h))
    jobs["flags"] = JOB_BIPRED
    jobs["key_offset"] = np.concatenate([[0], np.cumsum(w * h)[:-1]])
    keys = np.zeros(int((w * h).sum()), np.int16)
    for i, pattern in enumerate(("block4", "block4", "pair", "pair", "high", "low")):
        one = jobs[i:i + 1]
        assert len(synth.extreme_keys(rng, one, keys, 8, pattern)) == 1
    assert set(np.unique(keys).tolist()) == {-255, 510}
    for hadme in (1, 0):
        ctx = _ctx("d8", use_hadamard=hadme, nn_mode=1, qp=22, fast_inter_mode=1)
        try:
            setup(ctx, pics, keys)
            orc = oracle_for(pics, keys, 8, use_hadamard=hadme, nn_mode=1, fast_inter_mode=1)
            g = {"jobs": jobs, "results": orc.refine(jobs), "pictures": [pics[k] for k in sorted(pics)], "keys": keys,
                 "lambdas": np.asarray(LAMBDAS)}
            _frac_single_check(ctx, g, range(len(jobs)))
        finally:
            ctx.close()


def test_single8_range_checkerboard():
    """The 8-bit server kernel on a 0 / 255 checkerboard of period 1 under keys of -255 and 510."""
    _single8_range_case(synth.stress_picture(W, H, 8, "checker1"))


def test_single8_range_vertical_stripes():
    """Vertical 0 / 255 stripes of period 2: the horizontal filter at its extremes alone."""
    _single8_range_case(synth.stress_picture(W, H, 8, "vstripe2"))


# ---- integer search and its ring tail: fme_tz.hip ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tz_expected(name, bd, sr, fen):
    pics, jobs, ext, keys = tz_case(name, bd, sr)
    orc = oracle_for(pics, keys, bd, nn_mode=0, fast_inter_mode=fen)
    out, sad = orc.integer_search(jobs, ext)
    ring = ext.copy()
    ring["flags"] |= TZ_RING
    return out, sad, ring, orc.integer_search_ring(jobs, ring)


@pytest.mark.parametrize("fen", [0, 1, 3])
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("name,sr", [(n, 8) for n in REFINE_KINDS] + [("flat", 32)])
def test_integer_search_and_ring(name, sr, bd, fen):
    """fme_integer_search and fme_integer_search_ring: MV and SAD (the ring's nine NN inputs too) of
    every job, lambda 0 among the lambdas, 30 % bi-pred full searches, half of them on extreme keys.
    (A rejected job makes the host forms raise: the invalid count is 0.)"""
    from nnfme.runtime import FmeContext
    pics, jobs, ext, keys = tz_case(name, bd, sr)
    out, sad, ring, (r_out, r_sad, r_nn) = _tz_expected(name, bd, sr, fen)
    ctx = FmeContext(nn_mode=0, fast_inter_mode=fen, bit_depth=bd)
    try:
        setup(ctx, pics, keys)
        got, gsad = ctx.integer_search(jobs, ext)
        rgot, rsad, rnn = ctx.integer_search_ring(jobs, ring)
    finally:
        ctx.close()
    what = f"{name} SearchRange {sr}, {bd} bits, FEN {fen}"
    bad = (got["mv_x"] != out["mv_x"]) | (got["mv_y"] != out["mv_y"]) | (gsad != sad)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} jobs differ from the oracle (first {int(np.flatnonzero(bad)[0])})"
    g, case = load_stress(f"tz{bd}"), f"{name}.sr{sr}"
    if case in g["sets"]:
        mv = g[f"{case}.mv_fen{fen}"]
        assert np.array_equal(got["mv_x"], mv[:, 0]) and np.array_equal(got["mv_y"], mv[:, 1])
        assert np.array_equal(gsad, g[f"{case}.sad_fen{fen}"])
    bad = (rgot["mv_x"] != r_out["mv_x"]) | (rgot["mv_y"] != r_out["mv_y"]) | (rsad != r_sad) | (rnn != r_nn).any(axis=1)
    assert not bad.any(), f"{what}, ring: {int(bad.sum())} of {len(bad)} jobs differ (first {int(np.flatnonzero(bad)[0])})"


# ---- cost surface, prediction error / merge estimate, SSE / skip estimate ------------------------------
@functools.lru_cache(maxsize=None)
def _surfaces(name, bd):
    pics, jobs, keys = surface_jobs(name, bd)
    return surface.surfaces_numpy(pics, keys, LAMBDAS, jobs, 1, bd)


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("name", SMALL_SETS)
def test_cost_surface(name, bd):
    from nnfme.runtime import FmeContext
    pics, jobs, keys = surface_jobs(name, bd)
    want = _surfaces(name, bd)
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, qp=22, fast_inter_mode=1, bit_depth=bd)
    try:
        setup(ctx, pics, keys)
        surf, pick = surface.cost_surface(ctx, jobs)
        assert surface.cost_surface_invalid_count(ctx) == 0
    finally:
        ctx.close()
    for f in ("dist", "cost"):
        bad = np.argwhere(surf[f] != want[f])
        assert bad.size == 0, (f, bad[:10], surf[f][tuple(bad[:10].T)], want[f][tuple(bad[:10].T)])
    assert (pick["status"] == 0).all()
    assert pick.tobytes() == surface.pick_numpy(want).tobytes()


def _merge_requests(rng, n):
    """Merge-estimation requests on a W x H picture: every shape but 64x64, 1..5 candidates drawn
    near one motion, the ME motion present for three in four."""
    shapes = [s for s in synth.ALL_PU_SIZES if s != (64, 64)]
    reqs = np.zeros(n, merge.MERGE_REQ_DTYPE)
    for i, q in enumerate(reqs):
        w, h = shapes[i % len(shapes)]
        x, y = 4 * int(rng.integers(0, (W - w) // 4 + 1)), 4 * int(rng.integers(0, (H - h) // 4 + 1))
        q["x"], q["y"], q["w"], q["h"] = x, y, w, h
        q["cu_x"], q["cu_y"] = merge.cu_origin(x, y, w, h)
        q["cu_w"] = synth.cu_size_for(w, h)
        q["org_id"], q["lambda_id"] = 4, i % 4
        k = 1 + i % 5
        q["n_cand"] = q["max_num_merge_cand"] = k
        near = rng.integers(-40, 41, 2)
        motions = []
        for _ in range(k + 1):
            d = int(rng.integers(1, 4))
            ref, mv = np.zeros(2, np.uint8), np.zeros((2, 2), np.int16)
            for l in range(2):
                if d & (1 << l):
                    ref[l], mv[l] = int(rng.integers(0, 4)), near + rng.integers(-6, 7, 2)
            motions.append((d, ref, mv))
        for c, (d, ref, mv) in zip(q["cand"], motions):
            c["inter_dir"], c["ref_id"], c["mv"] = d, ref, mv
        if i % 4 != 3:
            q["flags"] |= merge.MRG_HAS_ME
            q["me_inter_dir"], q["me_ref_id"], q["me_mv"] = motions[k]
            q["me_bits"] = int(rng.integers(2, 30))
    return reqs


@functools.lru_cache(maxsize=None)
def _merge_expected(name, bd):
    pics, tasks = merge_case(name, bd)
    dist = np.array([merge.pred_error_numpy(pics, t, 1, bd) for t in tasks], np.uint32)
    reqs = _merge_requests(np.random.default_rng(1500 + bd), 46)
    rtasks, first = merge.expand_requests(reqs)
    rdist = np.array([merge.pred_error_numpy(pics, t, 1, bd) for t in rtasks], np.uint32)
    res = np.zeros(len(reqs), merge.MERGE_RES_DTYPE)
    for i, q in enumerate(reqs):
        res[i] = merge.merge_decide_numpy(q, rdist[first[i]:], 65536.0 * np.sqrt(LAMBDAS[int(q["lambda_id"])]))
    return dist, reqs, res


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("name", SMALL_SETS)
def test_pred_error_and_merge_estimate(name, bd):
    from nnfme.runtime import FmeContext
    pics, tasks = merge_case(name, bd)
    want, reqs, want_res = _merge_expected(name, bd)
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=bd)
    try:
        setup(ctx, pics)
        dist = merge.pred_error(ctx, tasks)
        assert merge.pred_error_invalid_count(ctx) == 0
        res = merge.merge_estimate(ctx, reqs)   # an invalid request makes it raise
    finally:
        ctx.close()
    bad = np.flatnonzero(dist != want)
    assert bad.size == 0, (bad[:10], dist[bad[:10]], want[bad[:10]], tasks[bad[:10]])
    for f in merge.MERGE_RES_DTYPE.names:
        bad = np.flatnonzero((res[f] != want_res[f]).reshape(len(res), -1).any(axis=1))
        assert bad.size == 0, (f, bad[:10], res[f][bad[:10]], want_res[f][bad[:10]])


def _skip_requests(rng, n):
    """Skip requests: CUs of 8..64, 0..5 candidates near one motion, all evaluated, bits 1..40; every
    third repeats a candidate (an exact cost tie)."""
    reqs = np.zeros(n, skip.SKIP_REQ_DTYPE)
    for i, q in enumerate(reqs):
        s = (8, 16, 32, 64)[i % 4]
        q["x"], q["y"] = s * int(rng.integers(0, W // s)), s * int(rng.integers(0, MC_H // s))
        q["w"] = q["h"] = s
        q["org_id"] = 3
        k = (i // 4) % 6
        q["n_cand"], q["cand_mask"] = k, (1 << k) - 1
        near = rng.integers(-40, 41, 2)
        for c in range(k):
            d = int(rng.integers(1, 4))
            q["cand"][c]["inter_dir"] = d
            for l in range(2):
                if d & (1 << l):
                    q["cand"][c]["ref_id"][l] = int(rng.integers(0, 3))
                    q["cand"][c]["mv"][l] = near + rng.integers(-10, 11, 2)
            q["bits"][c] = int(rng.integers(1, 41))
        if i % 3 == 1 and k >= 2:
            q["cand"][k - 1], q["bits"][k - 1] = q["cand"][0], q["bits"][0]
    return reqs


@functools.lru_cache(maxsize=None)
def _skip_case(kind, bd):
    """(4:2:0 pictures, tasks, their [Y, Cb, Cr] SSEs, requests, their results): the predictions are
    the oracle's motion compensation, the sums skip.block_sse, the decision skip_decide_numpy."""
    from oracle import Oracle
    pics = synth.stress_yuv(W, MC_H, bd, kind, slots=4)
    if kind == "full":   # full against zero: the original (slot 3) at 0
        pics[3] = tuple(np.zeros_like(p) for p in pics[3])
    rng = np.random.default_rng(1600 + bd)
    shapes = np.array(synth.ALL_PU_SIZES)[np.arange(72) % 24]
    tasks = np.zeros(72, skip.SSE_TASK_DTYPE)
    tasks["w"], tasks["h"] = shapes[:, 0], shapes[:, 1]
    tasks["x"] = rng.integers(0, (W - shapes[:, 0]) // 4 + 1) * 4
    tasks["y"] = rng.integers(0, (MC_H - shapes[:, 1]) // 4 + 1) * 4
    cu = np.array([merge.cu_origin(*v) for v in zip(tasks["x"], tasks["y"], tasks["w"], tasks["h"])])
    tasks["cu_x"], tasks["cu_y"] = cu[:, 0], cu[:, 1]
    tasks["org_id"] = 3
    tasks["flags"] = rng.integers(1, 4, 72)
    tasks["ref_id"] = rng.integers(0, 3, (72, 2))
    amp = np.where(rng.random(72) < 0.1, 600, 70)[:, None, None]
    tasks["mv"] = (rng.integers(-1000, 1001, (72, 2, 2)) * amp) // 1000
    for l in range(2):
        unused = (tasks["flags"] & (1 << l)) == 0
        tasks["ref_id"][unused, l] = 0
        tasks["mv"][unused, l] = 0
    orc = Oracle(bit_depth=bd)
    dt = pics[0][0].dtype

    def sse_of(ts):
        out = np.zeros((len(ts), 3), np.uint32)
        pred = (np.zeros((MC_H, W), dt), np.zeros((MC_H // 2, W // 2), dt), np.zeros((MC_H // 2, W // 2), dt))
        jobs = np.zeros(len(ts), MC_JOB_DTYPE)
        for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv", "flags"):
            jobs[f] = ts[f]
        for i, t in enumerate(ts):
            orc.mc(pics, jobs[i:i + 1], *pred)
            out[i] = skip.block_sse(pics[3], pred, t, bd)
        return out

    reqs = _skip_requests(rng, 48)
    params = skip.make_params(LAMBDAS[1], (0.75, 1.25))
    rtasks, first = skip.expand_requests(reqs)
    rsse = sse_of(rtasks)
    res = np.zeros(len(reqs), skip.SKIP_RES_DTYPE)
    for i, q in enumerate(reqs):
        res[i] = skip.skip_decide_numpy(q, rsse[first[i]:], params)
    return pics, tasks, sse_of(tasks), reqs, params, res


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("kind", ["checker1", "binary", "full", "flat"])
def test_pred_sse_and_skip_estimate(kind, bd):
    """Luma and chroma planes of the same kind (`full`: references at max against an original at 0,
    every 64x64 sum at its ceiling)."""
    from nnfme.runtime import FmeContext
    pics, tasks, want, reqs, params, want_res = _skip_case(kind, bd)
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=bd)
    try:
        for k, v in pics.items():
            ctx.set_picture_yuv(k, *v)
        got = skip.pred_sse(ctx, tasks)
        assert skip.pred_sse_invalid_count(ctx) == 0
        res = skip.skip_estimate(ctx, params, reqs)   # an invalid request makes it raise
    finally:
        ctx.close()
    for c, comp in enumerate(("Y", "Cb", "Cr")):
        bad = np.flatnonzero(got[:, c] != want[:, c])
        assert bad.size == 0, (comp, bad[:10], got[bad[:10]], want[bad[:10]], tasks[bad[:10]])
    if kind == "full":
        big = (tasks["w"] == 64) & (tasks["h"] == 64)
        assert big.any() and (got[big, 0] == (hi_of(bd) ** 2 >> (2 * (bd - 8))) * 4096).all()
    assert res.tobytes() == want_res.tobytes()


# ---- motion compensation: fme_mc.hip -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uni", "bi", "wp"])
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("kind", ["binary", "checker1", "full"])
def test_motion_compensate(kind, bd, mode):
    """Uni, bi and explicit WP at the table's extremes, MVs out to +-600 quarter-pels, against
    oracle/_ref's planes (the only 10-bit WP reference)."""
    from nnfme.runtime import FmeContext
    pics, jobs, wp, want = mc_case(load_stress(f"mc{bd}"), kind, mode, bd)
    assert all(mc_clip_bites(jobs))
    ctx = FmeContext(nn_mode=0, bit_depth=bd)
    try:
        for k, v in pics.items():
            ctx.set_picture_yuv(k, *v)
        if wp is not None:
            for l in range(2):
                for r in range(wp.shape[1]):
                    ctx.set_wp(l, r, wp[l, r])
        got = tuple(np.zeros_like(p) for p in want)
        ctx.motion_compensate(jobs, *got)   # an invalid job makes it raise
        assert ctx.mc_invalid_count() == 0
    finally:
        ctx.close()
    for a, b, comp in zip(got, want, ("Y", "Cb", "Cr")):
        assert np.array_equal(a, b), f"{kind} {mode} {bd} bits, {comp}: {int((a != b).sum())} samples differ"


# ---- the producers: bi-pred keys, template costs, predInterSearch on P and B slices ----------------------
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("name", ["full-zero", "zero-full", "binary"])
def test_device_bipred_keys_then_refine(name, bd, clip):
    """fme_build_bipred_keys where the keys reach -(2^b - 1) and 2 (2^b - 1) (0 and 2^b - 1 with the
    clip): refinements on the device-built keys equal the same jobs on the fixture's keys
    (oracle/_ref's removeHighFreq; at 8 bits also synth.bipred_keys) and the oracle's records."""
    g = load_stress(f"bikey{bd}")
    pics = case_pictures(g, name, name, bd)
    jobs, reqs, keys = g[f"{name}.jobs"], g[f"{name}.reqs"].copy(), g[f"{name}.keys_clip{clip}"]
    reqs["flags"] = abi.PU_CLIP_BIPRED if clip else 0
    if bd == 8:
        assert np.array_equal(synth.bipred_keys(reqs, pics, len(keys)), keys)
    if name == "full-zero":     # 2 * max - 0: the top of the range, clipped to max
        assert (keys == (hi_of(bd) if clip else 2 * hi_of(bd))).all()
    elif name == "zero-full":   # 2 * 0 - max: the bottom, clipped to 0
        assert (keys == (0 if clip else -hi_of(bd))).all()
    want = oracle_for(pics, keys, bd, use_hadamard=1, nn_mode=1, fast_inter_mode=1).refine(jobs)
    dev, host = (_ctx("d8" if bd == 8 else "d10", use_hadamard=1, nn_mode=1, qp=22, fast_inter_mode=1) for _ in range(2))
    try:
        setup(dev, pics)
        setup(host, pics, keys)
        dev.build_bipred_keys(reqs, len(keys))
        a, b = dev.refine(jobs), host.refine(jobs)
        assert dev.refine_status() == 0 and host.refine_status() == 0
    finally:
        dev.close()
        host.close()
    assert a.tobytes() == b.tobytes()
    _same_records(a, want, f"{name} {bd} bits clip {clip}")


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("name", PRODUCER_KINDS)
def test_template_costs(name, bd):
    from nnfme.runtime import FmeContext
    g = load_stress(f"template{bd}")
    pics = case_pictures(g, name, name, bd, height=MC_H)
    ctx = FmeContext(nn_mode=0, bit_depth=bd)
    try:
        setup(ctx, pics)
        got = ctx.template_costs(g[f"{name}.reqs"])
    finally:
        ctx.close()
    bad = np.argwhere(got != g[f"{name}.cost"])
    assert bad.size == 0, (bad[:10], got[tuple(bad[:10].T)], g[f"{name}.cost"][tuple(bad[:10].T)])


def _compare_all(got, exp, dtype):
    for f in dtype.names:
        if f.startswith("reserved"):
            continue
        bad = got[f] != exp[f]
        if bad.ndim > 1:
            bad = bad.reshape(len(bad), -1).any(axis=1)
        assert not bad.any(), f"{f}: {int(bad.sum())} of {len(bad)} requests differ (first {int(np.flatnonzero(bad)[0])})"


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("kind", PRODUCER_KINDS)
def test_pred_inter_p(kind, bd):
    """The AMVP pick, the reference choice and xCheckBestMVP on dense ties; two calls, so that
    m_integerMv2Nx2N and the NN state cross them."""
    from nnfme.runtime import FmeContext
    pics, reqs, exp, state = pred_inter_p_case(kind, bd)
    ctx = FmeContext(nn_mode=1, qp=22, fast_inter_mode=1, bit_depth=bd)
    try:
        setup(ctx, pics)
        cut = len(reqs) // 3 + 7
        got = np.concatenate([ctx.pred_inter_p(reqs[:cut]), ctx.pred_inter_p(reqs[cut:])])
        after = ctx.nn_get_state()
    finally:
        ctx.close()
    _compare_all(got, exp, abi.PU_RES_DTYPE)
    assert np.array_equal(after, state)


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("kind", PRODUCER_KINDS)
def test_pred_inter_b(kind, bd):
    """B slices with one shared reference: the uni / bi decision and the bi-pred iterations."""
    from nnfme.runtime import FmeContext
    from test_pred_inter_b import _compare
    pics, reqs, exp, state = pred_inter_b_case(kind, bd)
    ctx = FmeContext(nn_mode=1, qp=22, fast_inter_mode=1, bit_depth=bd)
    try:
        setup(ctx, pics)
        got = ctx.pred_inter_b(reqs)
        after = ctx.nn_get_state()
    finally:
        ctx.close()
    _compare(got, exp)
    assert np.array_equal(after, state)
