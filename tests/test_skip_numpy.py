"""The plain numpy restatement in nnfme/skip.py (getDistPart with DF_SSE, the chroma weighting, the
RD cost, the strict masked minimum) against the skip fixtures (tools/gen_skip_golden.py: the
predictions are the reference's own TLibCommon), and against direct definitions (CPU only).  The
GPU tests use the restatement for their live checks."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nnfme import skip, synth

FIXTURES = ("skip8", "skip10")


def load_skip_golden(name):
    return dict(np.load(os.path.join(GOLDEN, "skip", name + ".npz"), allow_pickle=False))


@pytest.fixture(scope="module", params=FIXTURES)
def fixture(request):
    return request.param, load_skip_golden(request.param)


def _used_mvs(t):
    """The MV of each task's first predicted list."""
    fl = t["flags"] & 3
    return t["mv"][np.arange(len(t)), np.where(fl == 2, 1, 0)].astype(np.int32)


def test_fixture_coverage(fixture):
    name, g = fixture
    bd = int(g["bit_depth"][0])
    assert bd == (10 if name == "skip10" else 8)
    assert g["y"].shape == (3, 96, 128) and g["cb"].shape == g["cr"].shape == (3, 48, 64)
    assert g["y"].dtype == g["cb"].dtype == (np.uint16 if bd > 8 else np.uint8)
    for c in ("cb", "cr"):   # textured chroma
        assert all(len(np.unique(p)) > 32 for p in g[c])
    t = g["tasks"]
    assert g["sse"].shape == (len(t), 3) and g["sse"].dtype == np.uint32
    assert {(int(a), int(b)) for a, b in zip(t["w"], t["h"])} == {tuple(s) for s in synth.ALL_PU_SIZES}
    mv = _used_mvs(t)
    for shape in synth.ALL_PU_SIZES:
        m = (t["w"] == shape[0]) & (t["h"] == shape[1])
        assert m.sum() == 64
        fl = t["flags"][m] & 3
        assert {1, 2, 3} <= set(fl.tolist())
        bi = t[m][fl == 3]
        same = (bi["ref_id"][:, 0] == bi["ref_id"][:, 1]) & (bi["mv"][:, 0] == bi["mv"][:, 1]).all(axis=1)
        assert same.any() and (~same).any()   # identical motion and true bi-prediction
        assert len({(int(a) & 7, int(b) & 7) for a, b in mv[m]}) == 64   # every chroma eighth-pel phase
        assert len({(int(a) & 3, int(b) & 3) for a, b in mv[m]}) == 16   # every luma quarter-pel phase
        corners = {(0, 0), (128 - shape[0], 0), (0, 96 - shape[1]), (128 - shape[0], 96 - shape[1])}
        assert corners <= {(int(a), int(b)) for a, b in zip(t["x"][m], t["y"][m])}
        assert (np.abs(t["mv"][m].astype(np.int32)) > 4 * 128).any()   # MVs that clipMv changes
    q, r = g["reqs"], g["res"]
    assert set(q["w"].tolist()) == {8, 16, 32, 64} and (q["w"] == q["h"]).all()
    for s in (8, 16, 32, 64):
        pos = {(int(a), int(b)) for a, b in zip(q["x"][q["w"] == s], q["y"][q["w"] == s])}
        assert {(0, 0), (128 - s, 0), (0, 96 - s), (128 - s, 96 - s)} <= pos and len(pos) > 4
    assert set(q["n_cand"].tolist()) == set(range(6))
    ev = np.array([skip.eval_mask(x) for x in q])
    full = (1 << q["n_cand"].astype(np.int32)) - 1
    assert ((ev == 0) & (q["n_cand"] > 0)).any()                       # the empty mask
    assert ((ev == full) & (q["n_cand"] == 5)).any()                   # all five
    assert any(bin(e).count("1") == 1 and n > 1 for e, n in zip(ev, q["n_cand"]))   # a single one of several
    assert ((r["best"] == skip.SKIP_NONE) == (ev == 0)).all()
    b = q["bits"][np.arange(5)[None, :] < q["n_cand"][:, None]]
    assert b.min() >= 1 and b.max() <= 40 and len(np.unique(b)) > 30
    ties = 0
    for x in r:   # the least cost twice: the first stays
        c = x["cand_cost"]
        k = int(x["best"])
        if k != skip.SKIP_NONE and (c[k + 1:] == c[k]).any():
            ties += 1
            assert (c[:k] > c[k]).all()
    assert ties >= 5
    w = g["params"]["chroma_weight"]
    want = {1.0, 2.0 ** (-1.0 / 3.0), 2.0 ** (2.0 / 3.0), 1.2599}
    assert set(w[:, 0].tolist()) == want and set(w[:, 1].tolist()) == want
    lam = {float(v) for qp in synth.LDP_LAMBDA.values() for v in qp}
    assert set(g["params"]["lambda"].tolist()) <= lam and len(set(g["params"]["lambda"].tolist())) >= 6
    assert set(g["req_slice"].tolist()) == set(range(len(g["params"])))


def test_numpy_decision_reproduces_fixture_results(fixture):
    name, g = fixture
    tasks, first = skip.expand_requests(g["reqs"])
    assert tasks.tobytes() == g["req_tasks"].tobytes()
    assert len(g["req_sse"]) == len(tasks)
    for i, q in enumerate(g["reqs"]):
        r = skip.skip_decide_numpy(q, g["req_sse"][first[i]:], g["params"][g["req_slice"][i]])
        assert r.tobytes() == g["res"][i].tobytes(), i


def test_fixture_sse_equals_reference_library(fixture):
    """The fixtures' SSEs again from oracle/_ref's motion compensation (where it is built)."""
    from oracle import REF_SO, Reference
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref is not built (needs the reference sources)")
    from nnfme.abi import MC_JOB_DTYPE
    name, g = fixture
    bd = int(g["bit_depth"][0])
    ref = Reference(bit_depth=bd)
    for k in range(3):
        ref.set_picture_yuv(k, g["y"][k], g["cb"][k], g["cr"][k])
    idx = np.arange(0, len(g["tasks"]), 5)
    jobs = np.zeros(1, MC_JOB_DTYPE)
    for i in idx:
        t = g["tasks"][i]
        for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv"):
            jobs[0][f] = t[f]
        jobs[0]["flags"] = t["flags"]
        pred = (np.zeros_like(g["y"][0]), np.zeros_like(g["cb"][0]), np.zeros_like(g["cr"][0]))
        ref.mc(jobs, *pred)
        assert skip.block_sse((g["y"][0], g["cb"][0], g["cr"][0]), pred, t, bd) == g["sse"][i].tolist(), i


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_sse_numpy_equals_direct_sum(bit_depth):
    rng = np.random.default_rng(bit_depth)
    hi = (1 << bit_depth) - 1
    s = (bit_depth - 8) << 1
    for w, h in list(synth.ALL_PU_SIZES) + [(2, 2), (32, 32)]:
        a = rng.integers(0, hi + 1, (h, w)).astype(np.uint16)
        b = rng.integers(0, hi + 1, (h, w)).astype(np.uint16)
        direct = int((((a.astype(np.int64) - b.astype(np.int64)) ** 2) >> s).sum())
        assert skip.sse_numpy(a, b, bit_depth) == direct
        if bit_depth > 8:   # each sample's square is shifted, not the sum
            assert direct <= int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) >> s
    # the extremes stay inside Distortion (UInt)
    z, f = np.zeros((64, 64), np.uint16), np.full((64, 64), hi, np.uint16)
    assert skip.sse_numpy(z, f, bit_depth) == 4096 * ((hi * hi) >> s) < 2 ** 32
    one = np.full((4, 4), 3, np.uint16)   # 10 bits: 9 >> 4 = 0 per sample, though the sum 144 >> 4 = 9
    assert skip.sse_numpy(one, np.zeros((4, 4), np.uint16), bit_depth) == (0 if bit_depth > 8 else 144)


def test_weighting_truncates():
    assert skip.weighted_numpy(1.0, 12345) == 12345
    assert skip.weighted_numpy(0.5, 7) == 3
    assert skip.weighted_numpy(2.0 ** (2.0 / 3.0), 1000) == int(2.0 ** (2.0 / 3.0) * 1000.0) == 1587
    w = (1000.0 - 5e-10) / 1000.0   # the product lands within 1e-9 below 1000
    assert 0.0 < 1000.0 - w * 1000.0 < 1e-9
    assert skip.weighted_numpy(w, 1000) == 999
    w = (3000000.0 - 8e-10) / 3000000.0
    assert 0.0 < 3000000.0 - w * 3000000.0 < 1e-9
    assert skip.weighted_numpy(w, 3000000) == 2999999
    # through the decision: Y + Cb' + Cr' in UInt arithmetic, cost in doubles, strict minimum
    q = np.zeros((), skip.SKIP_REQ_DTYPE)
    q["n_cand"], q["cand_mask"] = 3, 0b111
    q["cand"]["inter_dir"][:3] = 1
    q["bits"][:3] = (4, 4, 3)
    p = skip.make_params(10.0, (w, 0.5))
    r = skip.skip_decide_numpy(q, np.array([[100, 3000000, 7], [100, 3000000, 6], [110, 3000000, 7]], np.uint32), p)
    assert r["cand_dist"][:3].tolist() == [100 + 2999999 + 3, 100 + 2999999 + 3, 110 + 2999999 + 3]
    assert r["cand_cost"][:3].tolist() == [3000102.0 + 40.0, 3000102.0 + 40.0, 3000112.0 + 30.0]
    assert int(r["best"]) == 0 and r["best_cost"] == 3000142.0   # three equal costs: the first
    assert math.isinf(r["cand_cost"][3]) and r["cand_dist"][4] == skip.NO_SSE
    q["cand_mask"] = 0b110
    r = skip.skip_decide_numpy(q, np.array([[100, 3000000, 6], [110, 3000000, 7]], np.uint32), p)
    assert int(r["best"]) == 1 and r["cand_dist"][0] == skip.NO_SSE and (r["cand_sse"][0] == skip.NO_SSE).all()
    q["cand_mask"] = 0b11000   # only bits at and above n_cand: none
    r = skip.skip_decide_numpy(q, np.zeros((0, 3), np.uint32), p)
    assert int(r["best"]) == skip.SKIP_NONE and math.isinf(r["best_cost"])
    q["cand_mask"] = 0b1   # the sum wraps in UInt
    wrap = skip.skip_decide_numpy(q, np.array([[0xFFFFFFF0, 0x20, 0xA]], np.uint32), skip.make_params(0.0, (1.0, 0.5)))
    assert wrap["cand_dist"][0] == 0x15 and wrap["cand_cost"][0] == 21.0
