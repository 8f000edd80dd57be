"""The plain numpy restatements in nnfme/merge.py (xGetHADs / SAD, the luma prediction, the merge
decision) against the merge fixtures, which come from the reference's own TLibCommon
(tools/gen_merge_golden.py), and against the reference library itself where it is built (CPU only).
The GPU tests use these restatements for their live checks."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nnfme import merge, synth

FIXTURES = ("merge8_had", "merge8_sad", "merge10_had")


def load_merge_golden(name):
    return dict(np.load(os.path.join(GOLDEN, "merge", name + ".npz"), allow_pickle=False))


@pytest.fixture(scope="module", params=FIXTURES)
def fixture(request):
    return request.param, load_merge_golden(request.param)


def test_fixture_coverage(fixture):
    name, g = fixture
    t = g["tasks"]
    assert g["luma"].shape == (3, 96, 128)
    assert {(int(a), int(b)) for a, b in zip(t["w"], t["h"])} == {tuple(s) for s in synth.ALL_PU_SIZES}
    for shape in synth.ALL_PU_SIZES:
        m = (t["w"] == shape[0]) & (t["h"] == shape[1])
        fl = t["flags"][m] & 3
        assert {1, 2, 3} <= set(fl.tolist())
        bi = t[m][fl == 3]
        same = (bi["ref_id"][:, 0] == bi["ref_id"][:, 1]) & (bi["mv"][:, 0] == bi["mv"][:, 1]).all(axis=1)
        assert same.any() and (~same).any()   # identical motion and true bi-prediction
        used = t[m]["mv"][np.arange(m.sum()), np.where(fl == 2, 1, 0)]
        assert len({(int(a) & 3, int(b) & 3) for a, b in used}) == 16   # every quarter-pel phase
    corners = {(0, 0), (128 - 64, 0), (0, 96 - 64), (128 - 64, 96 - 64)}
    big = t[(t["w"] == 64) & (t["h"] == 64)]
    assert corners <= {(int(a), int(b)) for a, b in zip(big["x"], big["y"])}
    assert (np.abs(t["mv"].astype(np.int32)) > 4 * 128).any()   # MVs that clipMv changes
    lossless = (t["flags"] & merge.PE_LOSSLESS) != 0
    assert lossless.any() == (name == "merge8_had")
    q = g["reqs"]
    assert set(q["n_cand"].tolist()) == set(range(6)) and set(q["max_num_merge_cand"].tolist()) == {1, 2, 3, 4, 5}
    r = g["res"]
    assert ((q["flags"] & merge.MRG_HAS_ME) == 0).any() and r["use_merge"][(q["flags"] & merge.MRG_HAS_ME) == 0].all()
    assert ((r["merge_cost"] == r["me_cost"]) & (r["me_cost"] != merge.NO_COST)).any()   # MRG == ME: ME stays
    tie = [(np.sort(c[:n])[:2] if n >= 2 else [0, 1]) for c, n in zip(r["cand_cost"], q["n_cand"])]
    assert any(a == b for a, b in tie)   # two candidates with the least cost
    small = ((q["w"] == 8) & (q["h"] == 4)) | ((q["w"] == 4) & (q["h"] == 8))
    assert (small & (q["cu_w"] == 8) & (q["cand"]["inter_dir"] == 3).any(axis=1)).any()   # the bi-pred restriction


def test_numpy_restatement_reproduces_fixture_dist(fixture):
    name, g = fixture
    bd, had = int(g["bit_depth"][0]), int(g["use_hadamard"][0])
    lumas = {k: g["luma"][k] for k in range(3)}
    got = np.array([merge.pred_error_numpy(lumas, t, had, bd) for t in g["tasks"]], np.uint32)
    assert np.array_equal(got, g["dist"]), np.flatnonzero(got != g["dist"])[:10]
    got = np.array([merge.pred_error_numpy(lumas, t, had, bd) for t in g["req_tasks"]], np.uint32)
    assert np.array_equal(got, g["req_dist"])


def test_numpy_decision_reproduces_fixture_results(fixture):
    name, g = fixture
    tasks, first = merge.expand_requests(g["reqs"])
    assert tasks.tobytes() == g["req_tasks"].tobytes()
    ml = [65536.0 * np.sqrt(l) for l in g["lambdas"]]
    for i, q in enumerate(g["reqs"]):
        r = merge.merge_decide_numpy(q, g["req_dist"][first[i]:], ml[int(q["lambda_id"])])
        assert r.tobytes() == g["res"][i].tobytes(), i


def test_numpy_dist_equals_reference_library():
    """dist_numpy against TComRdCost::setDistParam + DistFunc of oracle/_ref on random blocks of
    every PU shape, Hadamard and SAD (where the reference library is built)."""
    from oracle import REF_SO, Reference
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref is not built (needs the reference sources)")
    ref = Reference()
    rng = np.random.default_rng(4)
    for w, h in synth.ALL_PU_SIZES:
        for hi in (255, 1023):
            org = rng.integers(0, hi + 1, (h, w)).astype(np.int16)
            cur = np.clip(org + rng.integers(-40, 41, (h, w)), 0, hi).astype(np.int16)
            for had in (True, False):
                assert merge.dist_numpy(org, cur, had) == ref.satd(org, cur, had), (w, h, hi, had)
