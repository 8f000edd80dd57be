"""Saturated, flat and two-level pictures on the CPU side (nnfme.synth.stress_picture, extreme_keys;
fixtures under tests/golden/stress/ from oracle/gen_golden.py).

Three things are checked here, none of which needs a GPU:
  * the C oracle (and oracle/_ref where it is built) reproduces every stress fixture;
  * the numpy mirrors that the surface, merge and skip GPU tests compare with agree with the oracle's
    own prediction (orc_pred_block) and distortions on this content, not only on smooth pictures;
  * the inputs do what they are for: the ties, the saturated predictions, the differences at the ends
    of their range and the near-ceiling sums that tests/test_gpu_stress.py relies on are present.

The case builders at the top are shared with tests/test_gpu_stress.py (computed once, read only)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nnfme import abi, merge, skip, surface, synth, weights
from nnfme.abi import JOB_BIPRED, JOB_EMI, JOB_LOSSLESS, compare_results
from oracle import REF_SO, Oracle, Reference

HAVE_REF = os.path.exists(REF_SO)
STRESS = os.path.join(GOLDEN, "stress")
W, H, MC_H = 128, 128, 64
LAMBDAS = synth.LDP_LAMBDA[22] + (0.0,)   # slot 4: lambda 0
DEPTHS = (8, 10)
REFINE_KINDS = ("checker1", "vstripe2", "hstripe2", "binary", "uniform", "full-zero", "flat", "full-flat", "twolevel",
                "blocks8")
SATURATING = ("checker1", "binary", "vstripe2")
L0 = [(0, 1), (1, 2)]     # B slices: (picture slot, POC distance) per reference index
L1 = [(5, -1), (1, 2)]    # L1 index 1 is L0 index 1: one shared reference


def hi_of(bit_depth):
    return (1 << bit_depth) - 1


@functools.lru_cache(maxsize=None)
def load_stress(name):
    return dict(np.load(os.path.join(STRESS, name + ".npz"), allow_pickle=False))


def case_pictures(g, case, name, bit_depth, height=H, slots=5):
    """The pictures of a fixture's case: the stored planes of a seeded set, else the regenerated ones."""
    if f"{case}.pictures" in g:
        return {k: p for k, p in enumerate(g[f"{case}.pictures"])}
    return synth.stress_pictures(W, height, bit_depth, name, slots)


def setup(eng, pics, keys=None, lambdas=LAMBDAS):
    for k, v in pics.items():
        eng.set_picture(k, v)
    for lid, lam in enumerate(lambdas):
        eng.set_lambda(lid, float(lam))
    if keys is not None and len(keys):
        eng.set_keys(keys)
    return eng


def oracle_for(pics, keys=None, bit_depth=8, lambdas=LAMBDAS, **cfg):
    orc = Oracle(bit_depth=bit_depth, qp=22, **cfg)
    if cfg.get("nn_mode", 1) == 1:
        orc.load_nn(weights.load_weights(22))
    return setup(orc, pics, keys, lambdas)


@functools.lru_cache(maxsize=None)
def refine_case(name, bit_depth):
    """(pictures, jobs, keys) of one refinement batch: the fixture's where it has the set, else built
    the way the fixtures' are."""
    g = load_stress(f"refine{bit_depth}")
    if name in g["sets"]:
        return case_pictures(g, name, name, bit_depth), g[f"{name}.jobs"], g[f"{name}.keys"]
    pics = synth.stress_pictures(W, H, bit_depth, name)
    rng = np.random.default_rng(750 + 10 * bit_depth + REFINE_KINDS.index(name))
    jobs, keys = synth.stress_refine_batch(rng, W, H, bit_depth, pics)
    return pics, jobs, keys


@functools.lru_cache(maxsize=None)
def refine_expected(name, bit_depth, hadme):
    """The oracle's records and its NN state after the batch (from a reset state)."""
    pics, jobs, keys = refine_case(name, bit_depth)
    orc = oracle_for(pics, keys, bit_depth, use_hadamard=hadme, nn_mode=1, fast_inter_mode=1)
    res = orc.refine(jobs)
    return res, orc.nn_get_state()


@functools.lru_cache(maxsize=None)
def tz_case(name, bit_depth, search_range=8):
    """(pictures, jobs, ext, keys) of one integer-search batch (fixture or built alike, 192 jobs)."""
    g = load_stress(f"tz{bit_depth}")
    case = f"{name}.sr{search_range}"
    if case in g["sets"]:
        return case_pictures(g, case, name, bit_depth), g[f"{case}.jobs"], g[f"{case}.ext"], g[f"{case}.keys"]
    pics = synth.stress_pictures(W, H, bit_depth, name)
    rng = np.random.default_rng(850 + 10 * bit_depth + REFINE_KINDS.index(name))
    jobs, ext, keys = synth.stress_tz_batch(rng, W, H, bit_depth, pics, calls_per_ctu=12, search_range=search_range)
    return pics, jobs, ext, keys


def producer_pictures(kind, bit_depth):
    return {k: synth.stress_picture(W, MC_H, bit_depth, kind, index=k) for k in range(6)}


@functools.lru_cache(maxsize=None)
def pred_inter_p_case(kind, bit_depth):
    """(pictures, fme_pu_req stream, the oracle's results, its NN state): 128x64, 64 -> 8 CUs, AMP,
    four references, 5 % lossless, NN on."""
    pics = producer_pictures(kind, bit_depth)
    reqs = synth.make_pu_requests(np.random.default_rng(1200 + bit_depth), W, MC_H, org_id=4, ref_ids=[0, 1, 2, 3],
                                  lambda_id=0, max_depth=3, lossless_frac=0.05)
    orc = oracle_for(pics, None, bit_depth, nn_mode=1, fast_inter_mode=1)
    return pics, reqs, orc.pred_inter_p(reqs), orc.nn_get_state()


@functools.lru_cache(maxsize=None)
def pred_inter_b_case(kind, bit_depth):
    """The same for a B slice: 2 + 2 references, one shared."""
    pics = producer_pictures(kind, bit_depth)
    reqs = synth.make_pu_requests_b(np.random.default_rng(1300 + bit_depth), W, MC_H, org_id=4, l0=L0, l1=L1,
                                    lambda_id=0, max_depth=3, lossless_frac=0.05)
    orc = oracle_for(pics, None, bit_depth, nn_mode=1, fast_inter_mode=1)
    return pics, reqs, orc.pred_inter_b(reqs), orc.nn_get_state()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_dist(orc, target, pred, hadamard, bit_depth):
    """The oracle's own distortion of one block: orc_satd / orc_sad, the PU's sum >> (bit_depth - 8)."""
    t = np.ascontiguousarray(target, np.int16)
    p = np.ascontiguousarray(pred, np.int16)
    h, w = t.shape
    d = orc.lib.orc_satd(_ptr(t), w, _ptr(p), w, w, h) if hadamard else orc.lib.orc_sad(_ptr(t), w, _ptr(p), w, w, h, 0)
    return d >> (bit_depth - 8)


def surface_jobs(name, bit_depth):
    """The surface inputs: rounds 0 and 1 of the refinement batch (every shape uni-pred and on
    extreme keys) and round 3's lossless jobs."""
    pics, jobs, keys = refine_case(name, bit_depth)
    sel = np.r_[0:48, np.flatnonzero(jobs["flags"] & JOB_LOSSLESS)]
    return pics, jobs[sel], keys


def merge_tasks(rng, n, bit_depth):
    """Prediction-error tasks on a W x H stress set: every shape, uni and bi, 15 % lossless, a tenth
    of the MVs far enough out for clipMv (tests/test_gpu_merge.py's stream with the shapes dealt out)."""
    shapes = np.array(synth.ALL_PU_SIZES)
    t = np.zeros(n, merge.PE_TASK_DTYPE)
    s = shapes[np.arange(n) % len(shapes)]
    t["w"], t["h"] = s[:, 0], s[:, 1]
    t["x"] = rng.integers(0, (W - s[:, 0]) // 4 + 1) * 4
    t["y"] = rng.integers(0, (H - s[:, 1]) // 4 + 1) * 4
    cu = np.array([merge.cu_origin(*v) for v in zip(t["x"], t["y"], t["w"], t["h"])])
    t["cu_x"], t["cu_y"] = cu[:, 0], cu[:, 1]
    t["org_id"] = 4
    t["flags"] = rng.integers(1, 4, n) | np.where(rng.random(n) < 0.15, merge.PE_LOSSLESS, 0)
    t["ref_id"] = rng.integers(0, 4, (n, 2))
    amp = np.where(rng.random(n) < 0.1, 600, 70)[:, None, None]
    t["mv"] = (rng.integers(-1000, 1001, (n, 2, 2)) * amp) // 1000
    for l in range(2):   # unused lists stay zero
        unused = (t["flags"] & (1 << l)) == 0
        t["ref_id"][unused, l] = 0
        t["mv"][unused, l] = 0
    return t


@functools.lru_cache(maxsize=None)
def merge_case(name, bit_depth):
    pics = synth.stress_pictures(W, H, bit_depth, name)
    return pics, merge_tasks(np.random.default_rng(1400 + bit_depth), 96, bit_depth)


# ---- the generators ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_stress_picture_kinds(bit_depth):
    hi, mid = hi_of(bit_depth), 1 << (bit_depth - 1)
    for kind in synth.STRESS_KINDS:
        p = synth.stress_picture(40, 24, bit_depth, kind, index=1)
        assert p.shape == (24, 40) and p.dtype == (np.uint16 if bit_depth > 8 else np.uint8)
        assert np.array_equal(p, synth.stress_picture(40, 24, bit_depth, kind, index=1))
        assert int(p.max()) <= hi
    y, x = np.mgrid[0:24, 0:40]
    assert np.array_equal(synth.stress_picture(40, 24, bit_depth, "checker1", 1), ((x + y + 1) & 1) * hi)
    assert np.array_equal(synth.stress_picture(40, 24, bit_depth, "vstripe2"), ((x >> 1) & 1) * hi)
    assert np.array_equal(synth.stress_picture(40, 24, bit_depth, "hstripe2"), ((y >> 1) & 1) * hi)
    assert np.array_equal(synth.stress_picture(40, 24, bit_depth, "blocks8", 2), mid + 40 * ((((x + 6) >> 3) + (y >> 3)) & 1))
    for kind, values in (("binary", {0, hi}), ("zero", {0}), ("full", {hi}), ("flat", {mid}), ("twolevel", {mid, mid + 1}),
                         ("checker4", {0, hi})):
        assert set(np.unique(synth.stress_picture(40, 24, bit_depth, kind)).tolist()) == values, kind
    u = synth.stress_picture(128, 128, bit_depth, "uniform")
    assert int(u.min()) == 0 and int(u.max()) == hi
    assert not np.array_equal(synth.stress_picture(40, 24, bit_depth, "binary", 0),
                              synth.stress_picture(40, 24, bit_depth, "binary", 1))
    with pytest.raises(ValueError):
        synth.stress_picture(8, 8, bit_depth, "sinusoid")
    s = synth.stress_pictures(16, 8, bit_depth, "full-zero")
    assert all(int(s[k].max()) == 0 for k in range(4)) and int(s[4].min()) == hi


@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_extreme_keys_patterns(bit_depth):
    hi = hi_of(bit_depth)
    jobs = np.zeros(6, abi.JOB_DTYPE)
    jobs["w"], jobs["h"] = 8, 4
    jobs["flags"] = [JOB_BIPRED] * 5 + [JOB_EMI]
    jobs["key_offset"] = [0, 32, 64, 96, 128, -1]
    keys = np.full(160, 7, np.int16)
    sel = synth.extreme_keys(np.random.default_rng(1), jobs, keys, bit_depth, synth.KEY_PATTERNS)
    assert sel.tolist() == [0, 1, 2, 3, 4]
    k = keys.reshape(5, 4, 8)
    assert set(np.unique(keys).tolist()) == {-hi, 2 * hi}
    assert len(np.unique(k[0])) == 2
    assert (k[1][:, :4] == -hi).all() and (k[1][:, 4:] == 2 * hi).all()
    assert k[2][0].tolist() == [-hi, -hi, 2 * hi, 2 * hi] * 2 and k[2][1].tolist() == [2 * hi, 2 * hi, -hi, -hi] * 2
    assert (k[3] == 2 * hi).all() and (k[4] == -hi).all()
    untouched = np.full(160, 7, np.int16)
    assert len(synth.extreme_keys(np.random.default_rng(1), jobs, untouched, bit_depth, "high", frac=0.0)) == 0
    assert (untouched == 7).all()


def test_stored_planes_are_the_generators():
    """The seeded planes in the fixtures are what stress_picture draws today."""
    for bit_depth in DEPTHS:
        g = load_stress(f"refine{bit_depth}")
        for name in ("binary", "twolevel"):
            want = synth.stress_pictures(W, H, bit_depth, name)
            assert all(np.array_equal(g[f"{name}.pictures"][k], want[k]) for k in range(5))


def test_fixture_files_are_small():
    sizes = {f: os.path.getsize(os.path.join(STRESS, f)) for f in os.listdir(STRESS)}
    assert len(sizes) == 10 and all(f.endswith(".npz") for f in sizes)
    assert max(sizes.values()) <= os.path.getsize(os.path.join(GOLDEN, "mc_shapes.npz")), sizes
    assert sum(sizes.values()) < 1_000_000, sizes


# ---- the oracle and oracle/_ref reproduce the fixtures ---------------------------------------------------
ENGINES = ("oracle", "ref")


def _engine(which, bit_depth, **cfg):
    if which == "ref":
        if not HAVE_REF:
            pytest.skip("oracle/_ref not built")
        e = Reference(bit_depth=bit_depth, **cfg)
    else:
        e = Oracle(bit_depth=bit_depth, qp=22, **cfg) if "nn_mode" in cfg else Oracle(bit_depth=bit_depth, **cfg)
    if cfg.get("nn_mode") == 1:
        e.load_nn(weights.load_weights(22))
    return e


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_refine_fixtures(bit_depth, which):
    g = load_stress(f"refine{bit_depth}")
    for name in g["sets"]:
        pics, jobs, keys = refine_case(str(name), bit_depth)
        for hadme in (1, 0):
            e = setup(_engine(which, bit_depth, use_hadamard=hadme, nn_mode=1, fast_inter_mode=1), pics, keys)
            bad, first, counts = compare_results(e.refine(jobs), g[f"{name}.results_hadme{hadme}"])
            assert bad == 0, f"{name}, HADME {hadme}: {bad} jobs differ (first {first}): {counts}"


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_integer_search_fixtures(bit_depth, which):
    g = load_stress(f"tz{bit_depth}")
    for case in g["sets"]:
        name, sr = str(case).split(".sr")
        pics, jobs, ext, keys = tz_case(name, bit_depth, int(sr))
        for fen in (0, 1, 3):
            e = setup(_engine(which, bit_depth, fast_inter_mode=fen), pics, keys)
            out, sad = e.integer_search(jobs, ext)
            mv = g[f"{case}.mv_fen{fen}"]
            bad = (out["mv_x"] != mv[:, 0]) | (out["mv_y"] != mv[:, 1]) | (sad != g[f"{case}.sad_fen{fen}"])
            assert not bad.any(), f"{case}, FEN {fen}: {int(bad.sum())} of {len(bad)} jobs differ"


def mc_case(g, kind, mode, bit_depth):
    """(reference pictures, jobs, WP table or None, expected planes) of one motion-compensation case."""
    if f"{kind}.ref_y" in g:
        pics = {k: (g[f"{kind}.ref_y"][k], g[f"{kind}.ref_cb"][k], g[f"{kind}.ref_cr"][k]) for k in range(3)}
    else:
        pics = synth.stress_yuv(W, MC_H, bit_depth, kind)
    case = f"{kind}.{mode}"
    want = tuple(g[f"{case}.pred_{c}"] for c in ("y", "cb", "cr"))
    return pics, g[f"{case}.jobs"], g.get(f"{case}.wp"), want


def mc_clip_bites(jobs):
    """(clipMv changes a used MV's x, the same for y) over 128x64 motion-compensation jobs."""
    used = np.stack([(jobs["flags"] & 1) != 0, (jobs["flags"] & 2) != 0], axis=1)
    cu_x, cu_y = jobs["cu_x"].astype(np.int64)[:, None], jobs["cu_y"].astype(np.int64)[:, None]
    mv_x, mv_y = jobs["mv"][:, :, 0].astype(np.int64), jobs["mv"][:, :, 1].astype(np.int64)
    return (bool(((synth._clip_cu_qpel(mv_x, cu_x, W) != mv_x) & used).any()),
            bool(((synth._clip_cu_qpel(mv_y, cu_y, MC_H) != mv_y) & used).any()))


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_mc_fixtures(bit_depth, which):
    """(The C oracle has no 10-bit weighted prediction: that case rests on oracle/_ref alone.)"""
    g = load_stress(f"mc{bit_depth}")
    n = 0
    for kind in g["kinds"]:
        for mode in g["modes"]:
            pics, jobs, wp, want = mc_case(g, str(kind), str(mode), bit_depth)
            assert len(jobs) >= 20 and all(mc_clip_bites(jobs)), (kind, mode)
            got = tuple(np.zeros_like(p) for p in want)
            e = _engine(which, bit_depth)
            if which == "ref":
                for k, v in pics.items():
                    e.set_picture_yuv(k, *v)
                if wp is not None:
                    for l in range(2):
                        for r in range(3):
                            e.set_wp(l, r, wp[l, r])
                e.mc(jobs, *got)
            elif wp is not None and bit_depth > 8:
                continue
            else:
                e.mc(pics, jobs, *got, wp=wp)
            for a, b, comp in zip(got, want, ("Y", "Cb", "Cr")):
                assert np.array_equal(a, b), f"{kind} {mode} {comp}: {int((a != b).sum())} samples differ"
            n += 1
    assert n == (9 if which == "ref" or bit_depth == 8 else 6)


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_bi_key_fixtures(bit_depth, which):
    g = load_stress(f"bikey{bit_depth}")
    hi = hi_of(bit_depth)
    lo_seen = hi_seen = False
    for name in g["sets"]:
        pics = case_pictures(g, str(name), str(name), bit_depth)
        e = setup(_engine(which, bit_depth), pics)
        reqs = g[f"{name}.reqs"]
        for clip in (0, 1):
            want = g[f"{name}.keys_clip{clip}"]
            for q in reqs:
                args = [int(q[f]) for f in ("org_id", "ref_id", "x", "y", "w", "h", "cu_x", "cu_y", "mv_x", "mv_y")]
                key = e.bi_key(*args, clip)
                off = int(q["key_offset"])
                assert np.array_equal(key.reshape(-1), want[off:off + key.size]), (name, clip, q)
            if clip:
                assert int(want.min()) >= 0 and int(want.max()) <= hi
            else:
                lo_seen |= int(want.min()) == -hi
                hi_seen |= int(want.max()) == 2 * hi
        if bit_depth == 8 and which == "oracle":   # the numpy restatement the GPU tests also compare with
            for clip in (0, 1):
                r = reqs.copy()
                r["flags"] = abi.PU_CLIP_BIPRED if clip else 0
                assert np.array_equal(synth.bipred_keys(r, pics, len(g[f"{name}.keys_clip{clip}"])), g[f"{name}.keys_clip{clip}"])
    assert lo_seen and hi_seen   # the keys reach both ends of the range include/fme.h states


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_template_cost_fixtures(bit_depth, which):
    g = load_stress(f"template{bit_depth}")
    for name in g["sets"]:
        pics = case_pictures(g, str(name), str(name), bit_depth, height=MC_H)
        e = setup(_engine(which, bit_depth, fast_inter_mode=1), pics)
        reqs, want = g[f"{name}.reqs"], g[f"{name}.cost"]
        for i, q in enumerate(reqs):
            for k in range(4):
                for m in range(2):
                    if m >= int(q["n_cand"][k]):
                        assert want[i, k, m] == 0xFFFFFFFF
                        continue
                    if which == "ref":
                        mx, my = (int(v) for v in q["cand"][k][m])
                        got = e.template_cost(4, int(q["ref_id"][k]), int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"]),
                                              int(q["cu_x"]), int(q["cu_y"]), mx, my, 1, int(q["lambda_id"]))
                    else:
                        got = e.template_cost(q, k, m)
                    assert got == want[i, k, m], (name, i, k, m)


# ---- the numpy mirrors on stress content -----------------------------------------------------------------
@pytest.mark.parametrize("bit_depth", DEPTHS)
@pytest.mark.parametrize("name", ["checker1", "binary", "full-zero", "flat"])
def test_surfaces_numpy_equals_oracle_distortions(name, bit_depth):
    """surfaces_numpy's 49 distortions per job against orc_pred_block + orc_satd / orc_sad, one job per
    shape uni-pred and one on extreme keys, plus the lossless ones."""
    pics, jobs, keys = surface_jobs(name, bit_depth)
    jobs = np.concatenate([jobs[:24], jobs[24:48:2], jobs[48:]])   # each shape uni-pred, half of them on keys
    orc = Oracle(bit_depth=bit_depth)
    surf = surface.surfaces_numpy(pics, keys, LAMBDAS, jobs, 1, bit_depth)
    for i, j in enumerate(jobs):
        x, y, w, h = (int(j[f]) for f in ("x", "y", "w", "h"))
        ko = int(j["key_offset"])
        target = keys[ko:ko + w * h].reshape(h, w) if ko >= 0 else pics[int(j["org_id"])][y:y + h, x:x + w]
        had = not int(j["flags"]) & JOB_LOSSLESS
        for dx, dy in ((0, 0), (-3, -3), (3, 3), (2, -1), (-2, 0), (0, 1), (1, 2)):
            pred = orc.pred_block(pics[int(j["ref_id"])], x, y, w, h, 4 * int(j["mv_x"]) + dx, 4 * int(j["mv_y"]) + dy)
            want = oracle_dist(orc, target, pred, had, bit_depth)
            assert surf["dist"][i, surface.index(dx, dy)] == want, (name, i, dx, dy)


@pytest.mark.parametrize("bit_depth", DEPTHS)
@pytest.mark.parametrize("name", ["checker1", "binary", "full-zero", "flat"])
def test_pred_error_numpy_equals_oracle_distortions(name, bit_depth):
    """merge.predict_numpy against orc_pred_block on the uni-pred tasks, and pred_error_numpy against
    the oracle's distortion of that prediction."""
    pics, tasks = merge_case(name, bit_depth)
    orc = Oracle(bit_depth=bit_depth)
    n = 0
    for t in tasks:
        if int(t["flags"]) & 3 == 3:
            continue
        l = 0 if int(t["flags"]) & 1 else 1
        x, y, w, h = (int(t[f]) for f in ("x", "y", "w", "h"))
        mx = int(synth._clip_cu_qpel(int(t["mv"][l][0]), int(t["cu_x"]), W))
        my = int(synth._clip_cu_qpel(int(t["mv"][l][1]), int(t["cu_y"]), H))
        pred = orc.pred_block(pics[int(t["ref_id"][l])], x, y, w, h, mx, my)
        assert np.array_equal(pred, merge.predict_numpy(pics, t, bit_depth)), (name, t)
        had = not int(t["flags"]) & merge.PE_LOSSLESS
        want = oracle_dist(orc, pics[4][y:y + h, x:x + w], pred, had, bit_depth)
        assert merge.pred_error_numpy(pics, t, 1, bit_depth) == want, (name, t)
        n += 1
    assert n >= 48


@pytest.mark.parametrize("bit_depth", DEPTHS)
@pytest.mark.parametrize("name", ["checker1", "binary", "full-zero"])
def test_block_sse_equals_oracle_sse(name, bit_depth):
    """skip.block_sse (luma) against the oracle's own SSE (orc_sse at 8 bits; per-sample (d * d) >> 4 at
    10) of orc_pred_block's prediction.  The largest sum is at least a quarter of the ceiling 64 * 64 *
    hi^2 (>> 4 at 10 bits) = 2.7e8: full against zero is the ceiling itself, and two independent
    {0, hi} planes differ in half their samples, of which sub-pel filtering may lose half again."""
    pics, tasks = merge_case(name, bit_depth)
    orc = Oracle(bit_depth=bit_depth)
    top = 0
    for t in tasks:
        if int(t["flags"]) & 3 == 3:
            continue
        l = 0 if int(t["flags"]) & 1 else 1
        x, y, w, h = (int(t[f]) for f in ("x", "y", "w", "h"))
        mx = int(synth._clip_cu_qpel(int(t["mv"][l][0]), int(t["cu_x"]), W))
        my = int(synth._clip_cu_qpel(int(t["mv"][l][1]), int(t["cu_y"]), H))
        pred = orc.pred_block(pics[int(t["ref_id"][l])], x, y, w, h, mx, my)
        full = np.zeros((H, W), np.int64)
        full[y:y + h, x:x + w] = pred
        got = skip.block_sse((pics[4],) * 3, (full,) * 3, t, bit_depth)[0]
        org = np.ascontiguousarray(pics[4][y:y + h, x:x + w], np.int16)
        if bit_depth == 8:
            orc.lib.orc_sse.restype = C.c_uint32
            want = orc.lib.orc_sse(_ptr(org), w, _ptr(np.ascontiguousarray(pred)), w, w, h)
        else:
            d = org.astype(np.int64) - pred
            want = int(((d * d) >> 4).sum())
        assert got == want, (name, t)
        top = max(top, got)
    assert top >= (64 * 64 * hi_of(bit_depth) ** 2 // 4) >> (2 * (bit_depth - 8)), top


# ---- the inputs do what they are for ---------------------------------------------------------------------
@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_flat_with_lambda_zero_ties_all_49(bit_depth):
    pics, jobs, keys = refine_case("flat", bit_depth)
    zero = (0.0,) * 5
    surf = surface.surfaces_numpy(pics, keys, zero, jobs, 1, bit_depth)
    assert (surf["cost"] == surf["cost"][:, :1]).all()
    res = oracle_for(pics, keys, bit_depth, zero, use_hadamard=1, nn_mode=0, fast_inter_mode=1).refine(jobs)
    for f in ("half_x", "half_y", "qtr_x", "qtr_y"):
        assert not res[f].any(), f
    assert np.array_equal(res["mv_x"], 4 * res["mv_int_x"]) and np.array_equal(res["mv_y"], 4 * res["mv_int_y"])


def tied_stages(surf):
    """Per job: (the half stage's minimum is reached by two of its nine candidates, the same for the
    quarter stage), on replay_search's candidate sets."""
    cost = surface._cost_rows(surf)
    r = surface.replay_search(surf)
    rows = np.arange(len(cost))
    zero = np.zeros(len(cost), np.int64)
    out = []
    for bx, by, step, order in ((zero, zero, 2, surface.REFINE_H),
                                (2 * r["half_x"].astype(np.int64), 2 * r["half_y"].astype(np.int64), 1, surface.REFINE_Q)):
        cand = np.stack([cost[rows, surface.index(bx + step * ox, by + step * oy)] for ox, oy in order], axis=1)
        out.append((cand == cand.min(axis=1, keepdims=True)).sum(axis=1) >= 2)
    return out


@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_flat_with_ldp_lambdas_ties_both_stages(bit_depth):
    """96 of 96 jobs: the half stage and the quarter stage each have a tied minimum (a smooth picture
    gives 13 of 96 at the half stage)."""
    pics, jobs, keys = refine_case("flat", bit_depth)
    res, _ = refine_expected("flat", bit_depth, 1)
    surf = surface.surfaces_numpy(pics, keys, LAMBDAS, surface.jobs_at_results(jobs, res), 1, bit_depth)
    half, qtr = tied_stages(surf)
    assert half.all() and qtr.all(), (int(half.sum()), int(qtr.sum()))
    r = surface.replay_search(surf)
    for f in ("half_x", "half_y", "qtr_x", "qtr_y", "frac_cost"):
        assert np.array_equal(r[f], res[f]), f


@pytest.mark.parametrize("bit_depth", DEPTHS)
@pytest.mark.parametrize("name", SATURATING)
def test_saturating_sets_reach_the_range_ends(name, bit_depth):
    """At the MVs the oracle returns: >= 1000 predicted samples at 0 and at hi (the clip after the
    second filter stage), a uni-pred difference of hi, and on the extreme keys a difference of
    2 * hi (2046 at 10 bits: the bound csrc/fme_lane10.hip states for its packed Hadamard)."""
    hi = hi_of(bit_depth)
    pics, jobs, keys = refine_case(name, bit_depth)
    res, _ = refine_expected(name, bit_depth, 1)
    orc = Oracle(bit_depth=bit_depth)
    at0 = athi = uni_top = key_top = 0
    for j, r in zip(jobs, res):
        x, y, w, h = (int(j[f]) for f in ("x", "y", "w", "h"))
        for qx, qy in {(int(r["mv_x"]), int(r["mv_y"])), (4 * int(r["mv_int_x"]) + 2, 4 * int(r["mv_int_y"]) + 2)}:
            pred = orc.pred_block(pics[int(j["ref_id"])], x, y, w, h, qx, qy).astype(np.int64)
            at0 += int((pred == 0).sum())
            athi += int((pred == hi).sum())
            ko = int(j["key_offset"])
            if ko >= 0:
                key_top = max(key_top, int(np.abs(keys[ko:ko + w * h].reshape(h, w).astype(np.int64) - pred).max()))
            else:
                uni_top = max(uni_top, int(np.abs(pics[4][y:y + h, x:x + w].astype(np.int64) - pred).max()))
    assert at0 >= 1000 and athi >= 1000, (at0, athi)
    assert uni_top == hi and key_top == 2 * hi, (uni_top, key_top)


@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_integer_search_on_binary_nears_the_ceiling(bit_depth):
    g = load_stress(f"tz{bit_depth}")
    top = max(int(g[f"binary.sr8.sad_fen{fen}"].max()) for fen in (0, 1, 3))
    assert top >= 2 * 10 ** 8, top
    jobs = g["binary.sr8.jobs"]
    assert 480 <= len(jobs) <= 640
    assert set(jobs["lambda_id"].tolist()) == {0, 1, 2, 3, 4}
    bi = (jobs["flags"] & JOB_BIPRED) != 0
    assert 0.2 < bi.mean() < 0.4
    keys = g["binary.sr8.keys"]
    assert int(keys.min()) == -hi_of(bit_depth) and int(keys.max()) == 2 * hi_of(bit_depth)


@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_producers_take_every_branch_on_ties(bit_depth):
    _, _, p, _ = pred_inter_p_case("flat", bit_depth)
    assert len(np.unique(p["ref_idx"])) >= 2 and set(np.unique(p["mvp_idx"]).tolist()) == {0, 1}
    _, _, b, _ = pred_inter_b_case("flat", bit_depth)
    assert {1, 2} <= set(np.unique(b["inter_dir"]).tolist())
    for kind in ("binary", "twolevel"):
        _, _, b, _ = pred_inter_b_case(kind, bit_depth)
        assert set(np.unique(b["inter_dir"]).tolist()) == {1, 2, 3}, kind


@pytest.mark.parametrize("bit_depth", DEPTHS)
def test_every_shape_and_flag_occurs(bit_depth):
    shapes = set(synth.ALL_PU_SIZES)
    _, jobs, _ = refine_case("binary", bit_depth)
    _, sjobs, _ = surface_jobs("binary", bit_depth)
    for j in (jobs, sjobs):
        assert set(zip(j["w"].tolist(), j["h"].tolist())) == shapes
        for flag in (JOB_EMI, JOB_BIPRED, JOB_LOSSLESS):
            assert (j["flags"] & flag).any(), flag
        assert ((j["flags"] & JOB_BIPRED) != 0).mean() >= 0.25
    _, tasks = merge_case("binary", bit_depth)
    assert set(zip(tasks["w"].tolist(), tasks["h"].tolist())) == shapes
    assert (tasks["flags"] & merge.PE_LOSSLESS).any() and {1, 2, 3} == set((tasks["flags"] & 3).tolist())
