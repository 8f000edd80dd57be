"""The cost surface restated in numpy (nnfme.surface.surface_numpy) on a CPU: against the fixtures
whose distortions are the reference's own primitives (tests/golden/surface, tools/gen_surface_golden.py),
and, replayed through xPatternRefinement's two stages, against the half / quarter picks and the
cost of the refinement goldens, which pin 17 of the 49 positions per job.  Every comparison is ==
on integers."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_bit_depth, load_golden
from nnfme import dataset, surface

FIXTURES = ("surf8", "surf10", "surf8_sad")
# refinement goldens: 8 and 10 bits, HAD and SAD, bi-pred keys, lossless jobs, all 24 shapes
REPLAY_GOLDENS = ("ldp_qp22_hadme_fen1_nn", "hadme_fen1_nnoff_qp22", "sad_fen0_nnoff", "fen3_qp27_nn", "ra_qp27_nn",
                  "main10_ldp_qp22_hadme_fen1_nn", "main10_sad_fen0_nnoff")
REPLAY_FIELDS = ("half_x", "half_y", "qtr_x", "qtr_y", "frac_cost")


def load_surface_golden(name):
    return dict(np.load(os.path.join(GOLDEN, "surface", name + ".npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def fixture_surfaces(name):
    """(fixture, surface_numpy of its jobs), computed once and shared (read only)."""
    g = load_surface_golden(name)
    s = surface.surfaces_numpy(g["pictures"], g["keys"], g["lambdas"], g["jobs"], int(g["config"][0]),
                               int(g["bit_depth"][0]))
    s.setflags(write=False)
    return g, s


def replay_with_wrong_order(cost):
    """replay_search with the H order in the quarter stage: what the replay must not be."""
    zero = np.zeros(len(cost), np.int64)
    hx, hy, _ = surface._stage(cost, zero, zero, 2, surface.REFINE_H)
    qx, qy, qc = surface._stage(cost, 2 * hx, 2 * hy, 1, surface.REFINE_H)
    return hx, hy, qx, qy, qc


def assert_replay(surf, results):
    r = surface.replay_search(surf)
    for f in REPLAY_FIELDS:
        bad = np.flatnonzero(r[f] != results[f])
        assert bad.size == 0, (f, bad[:10], r[f][bad[:10]], results[f][bad[:10]])


def order_matters(surf):
    """Jobs on whose surface the quarter stage in the H order would break a tie differently."""
    r = surface.replay_search(surf)
    _, _, qx, qy, _ = replay_with_wrong_order(surface._cost_rows(surf))
    return np.flatnonzero((qx != r["qtr_x"]) | (qy != r["qtr_y"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_surface_numpy_matches_fixture(name):
    g, s = fixture_surfaces(name)
    assert len(g["jobs"]) >= 350 and g["dist"].shape == (len(g["jobs"]), surface.POINTS)
    bad = np.argwhere(s["dist"] != g["dist"])
    assert bad.size == 0, (bad[:10], g["jobs"][bad[:10, 0]])
    # what the fixture is there for
    j = g["jobs"]
    assert len({(int(a), int(b)) for a, b in zip(j["w"], j["h"])}) == 24
    assert (j["key_offset"] >= 0).any()
    ph, pw = g["pictures"].shape[1:]
    assert (j["x"] == 0).any() and (j["y"] == 0).any()
    assert (j["x"].astype(int) + j["w"] == pw).any() and (j["y"].astype(int) + j["h"] == ph).any()


def test_fixtures_hold_lossless_jobs():
    assert all((load_surface_golden(n)["jobs"]["flags"] & 0x04).any() for n in FIXTURES)


def test_fixture_files_are_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, "surface", n + ".npz")) < largest


@pytest.mark.parametrize("name", REPLAY_GOLDENS)
def test_replay_reproduces_refinement_golden(name):
    """Every fourth job: the surface centred on mv_int, replayed, gives the reference's half and
    quarter offsets and its cost; the sample holds jobs that tell the Q order from the H order."""
    g = load_golden(name)
    jobs = surface.jobs_at_results(g["jobs"], g["results"])[::4]
    res = g["results"][::4]
    s = surface.surfaces_numpy(g["pictures"], g["keys"], g["lambdas"], jobs, int(g["config"][0]), golden_bit_depth(g))
    assert_replay(s, res)
    assert order_matters(s).size > 0


def test_index_is_the_nn_class_map():
    text = open(os.path.join(ROOT, "include", "fme_surface.h")).read()
    m = re.search(r"#define FME_SURF_INDEX\(dx, dy\) (.+)", text)
    assert m and "FME_SURF_POINTS 49" in text
    seen = set()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            i = int(surface.index(dx, dy))
            assert i == eval(m.group(1), {"dx": dx, "dy": dy})   # the header's macro
            assert surface.offset(i) == (dx, dy)                   # offset = (cls % 7 - 3, cls / 7 - 3)
            seen.add(i)
    assert seen == set(range(49))
    # OUT_CLASS of the training data (TEncSearch.cpp:4576-4578) for every half / quarter pair
    for hx in (-1, 0, 1):
        for hy in (-1, 0, 1):
            for qx in (-1, 0, 1):
                for qy in (-1, 0, 1):
                    assert int(dataset.out_class(hx, hy, qx, qy)) == int(surface.index(2 * hx + qx, 2 * hy + qy))


def test_pick_and_regret_on_arrays():
    rng = np.random.default_rng(5)
    cost = rng.integers(0, 6, (500, 49)).astype(np.uint32)   # few values: ties everywhere
    probes = rng.integers(0, 49, (500, 2)).astype(np.uint8)
    probes[::7, 1] = surface.NO_PROBE
    p = surface.pick_numpy(cost, probes)
    for i in range(500):
        first = min(range(49), key=lambda k: (int(cost[i, k]), k))
        assert p["min_idx"][i] == first and p["min_cost"][i] == cost[i, first]
        assert p["probe_cost"][i, 0] == cost[i, probes[i, 0]]
        assert p["probe_cost"][i, 1] == (surface.NO_COST if probes[i, 1] == surface.NO_PROBE else cost[i, probes[i, 1]])
    r = surface.replay_search(cost)
    res = np.zeros(500, [("half_x", "i1"), ("half_y", "i1"), ("qtr_x", "i1"), ("qtr_y", "i1"), ("nn_class", "u1")])
    for f in ("half_x", "half_y", "qtr_x", "qtr_y"):
        res[f] = r[f]
    res["nn_class"] = probes[:, 0]
    res["nn_class"][::5] = 255
    g = surface.regret(res, cost)
    assert (g["search_cost"] == r["frac_cost"]).all() and (g["min_cost"] == p["min_cost"]).all()
    assert (g["min_cost"] <= g["search_cost"]).all() and (g["min_idx"] == p["min_idx"]).all()
    assert (g["class_cost"][::5] == surface.NO_COST).all()
    keep = np.arange(500) % 5 != 0
    assert (g["class_cost"][keep] == cost[np.arange(500), probes[:, 0]][keep]).all()


def test_dataset_label_surface_min():
    g, s = fixture_surfaces("surf8")
    src = load_golden("ldp_qp22_hadme_fen1_nn")
    idx = g["src_index"]
    jobs, res = src["jobs"][idx], src["results"][idx]
    base, st = dataset.records(jobs, res)
    assert (base["y"] == dataset.out_class(res["half_x"], res["half_y"], res["qtr_x"], res["qtr_y"])).all()
    alt, st2 = dataset.records(jobs, res, label="surface_min", surface=s)
    assert (alt["y"] == np.argmin(s["cost"], axis=1)).all() and (st == st2).all()
    for f in base.dtype.names:
        if f != "y":
            assert (alt[f] == base[f]).all()
    assert (alt["y"] != base["y"]).any()   # the two-stage search misses the minimum on some jobs
    with pytest.raises(ValueError):
        dataset.records(jobs, res, label="surface_min")
    with pytest.raises(ValueError):
        dataset.records(jobs, res, label="nearest")
