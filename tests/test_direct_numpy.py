"""The NN-direct records restated in numpy (nnfme.direct.direct_numpy) on a CPU, no library needed.

On a job whose nn_class happens to be the position xPatternSearchFracDIF picked, index(2 half + qtr),
the shipped encoder's record already is the direct record: its frac_cost is the cost of the MV it
returns.  So on those jobs direct_numpy over surfaces_numpy must reproduce the goldens' mv, bits, cost
and frac_cost exactly, which pins the restated tail (and the surface at the class) to the reference's
own records.  Every comparison is == on integers."""
import functools

import numpy as np
import pytest

from conftest import golden_bit_depth, load_golden
from nnfme import direct, surface
from nnfme.abi import JOB_BIPRED, JOB_LOSSLESS, RES_NN_STALE, RES_NN_UNINIT, RES_REJECTED

NN_GOLDENS = ("ldp_qp22_hadme_fen1_nn", "fen3_qp27_nn", "qp32_nn", "qp37_nn", "ra_qp27_nn",
              "main10_ldp_qp22_hadme_fen1_nn", "main10_fen3_qp27_nn", "main10_ra_qp37_nn")
DEEP_GOLDENS = ("deep_master_qp22", "deep_scr3x40_qp22")
FIXTURES = NN_GOLDENS + DEEP_GOLDENS
PINNED = ("mv_x", "mv_y", "bits", "cost", "frac_cost")
CARRIED = ("mv_int_x", "mv_int_y", "c", "emi", "n_emi", "nn_class")

# (MVX_HALF, MVX_QRTER, MVY_HALF, MVY_QRTER) of the 49 cases of the switch at TEncSearch.cpp:136-193
SWITCH = (
    (-1, -1, -1, -1), (-1, 0, -1, -1), (0, -1, -1, -1), (0, 0, -1, -1), (0, 1, -1, -1), (1, 0, -1, -1), (1, 1, -1, -1),
    (-1, -1, -1, 0), (-1, 0, -1, 0), (0, -1, -1, 0), (0, 0, -1, 0), (0, 1, -1, 0), (1, 0, -1, 0), (1, 1, -1, 0),
    (-1, -1, 0, -1), (-1, 0, 0, -1), (0, -1, 0, -1), (0, 0, 0, -1), (0, 1, 0, -1), (1, 0, 0, -1), (1, 1, 0, -1),
    (-1, -1, 0, 0), (-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0),
    (-1, -1, 0, 1), (-1, 0, 0, 1), (0, -1, 0, 1), (0, 0, 0, 1), (0, 1, 0, 1), (1, 0, 0, 1), (1, 1, 0, 1),
    (-1, -1, 1, 0), (-1, 0, 1, 0), (0, -1, 1, 0), (0, 0, 1, 0), (0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 1, 0),
    (-1, -1, 1, 1), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1),
)


def agreeing(results):
    """Jobs whose class is the search's own pick."""
    at = surface.index(2 * results["half_x"].astype(np.int64) + results["qtr_x"],
                       2 * results["half_y"].astype(np.int64) + results["qtr_y"])
    return np.flatnonzero(results["nn_class"] == at)


@functools.lru_cache(maxsize=None)
def subset(name):
    """(fixture, sorted job indices, surfaces_numpy of those jobs centred on mv_int), computed once and
    shared (read only).  The seeded subset keeps every agreeing job, every lossless job, the first job
    of every PU shape and a few more (surfaces_numpy is slow for 64x64 PUs)."""
    g = load_golden(name)
    jobs, res = g["jobs"], g["results"]
    shapes = {}
    for i, (w, h) in enumerate(zip(jobs["w"], jobs["h"])):
        shapes.setdefault((int(w), int(h)), i)
    rng = np.random.default_rng(4000 + FIXTURES.index(name))
    small = np.flatnonzero(jobs["w"].astype(int) * jobs["h"] <= 512)
    idx = np.unique(np.r_[agreeing(res), np.flatnonzero(jobs["flags"] & JOB_LOSSLESS), list(shapes.values()),
                          rng.choice(small, 12, replace=False)])
    at = surface.jobs_at_results(jobs[idx], res[idx])
    s = surface.surfaces_numpy(g["pictures"], g["keys"], g["lambdas"], at, int(g["config"][0]), golden_bit_depth(g))
    s.setflags(write=False)
    idx.setflags(write=False)
    return g, idx, s


def test_half_qtr_of_class_is_the_switch():
    assert len(SWITCH) == 49
    hx, qx, hy, qy = direct.half_qtr_of_class(np.arange(49))
    for c in range(49):
        assert (int(hx[c]), int(qx[c]), int(hy[c]), int(qy[c])) == SWITCH[c], c
        # the globals recombine to the class's offset, which is what rcMv gets (TEncSearch.cpp:4590-4591)
        assert (2 * SWITCH[c][0] + SWITCH[c][1], 2 * SWITCH[c][2] + SWITCH[c][3]) == (c % 7 - 3, c // 7 - 3)
        one = direct.half_qtr_of_class(c)
        assert tuple(int(v) for v in one) == SWITCH[c]


def test_status_bit_is_its_own():
    assert direct.RES_NN_DIRECT == 0x04
    assert direct.RES_NN_DIRECT & (RES_NN_STALE | RES_NN_UNINIT | RES_REJECTED) == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_has_what_the_checks_need(name):
    g = load_golden(name)
    jobs, res = g["jobs"], g["results"]
    assert len(agreeing(res)) >= 10
    assert len(np.unique(res["nn_class"])) >= 30 and int(res["nn_class"].max()) < 49
    assert int((jobs["key_offset"] >= 0).sum()) >= 50
    assert int(((jobs["flags"] & JOB_LOSSLESS) != 0).sum()) == 16
    assert len({(int(w), int(h)) for w, h in zip(jobs["w"], jobs["h"])}) == 24
    assert int(g["config"][2]) in (1, 2)
    _, idx, _ = subset(name)
    sub = jobs[idx]
    assert len({(int(w), int(h)) for w, h in zip(sub["w"], sub["h"])}) == 24
    assert set(agreeing(res)) <= set(idx) and set(np.flatnonzero(jobs["flags"] & JOB_LOSSLESS)) <= set(idx)
    assert ((sub["flags"] & JOB_BIPRED) != 0).any() and (sub["key_offset"] >= 0).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_direct_numpy_reproduces_the_golden_where_the_class_is_the_pick(name):
    g, idx, surf = subset(name)
    jobs, res = g["jobs"][idx], g["results"][idx]
    exp = direct.direct_numpy(jobs, res, surf, g["lambdas"])
    agree = agreeing(res)
    assert len(agree) >= 10
    for f in PINNED:
        bad = agree[exp[f][agree] != res[f][agree]]
        assert bad.size == 0, (name, f, idx[bad][:10], exp[f][bad][:10], res[f][bad][:10])
    # on every job of the subset: what carries over, what the class alone decides, the new status bit
    for f in CARRIED:
        assert np.array_equal(exp[f], res[f]), f
    assert np.array_equal(exp["status"], res["status"] | direct.RES_NN_DIRECT)
    cls = res["nn_class"].astype(np.int64)
    assert np.array_equal(exp["mv_x"], 4 * res["mv_int_x"].astype(np.int64) + cls % 7 - 3)
    assert np.array_equal(exp["mv_y"], 4 * res["mv_int_y"].astype(np.int64) + cls // 7 - 3)
    assert np.array_equal(exp["mv_x"], res["mv_x"]) and np.array_equal(exp["mv_y"], res["mv_y"])
    assert np.array_equal(2 * exp["half_x"].astype(int) + exp["qtr_x"], cls % 7 - 3)
    assert np.array_equal(2 * exp["half_y"].astype(int) + exp["qtr_y"], cls // 7 - 3)
    assert np.array_equal(exp["frac_cost"], surface.regret(res, surf)["class_cost"])
    # bits do not depend on the cost: the golden's bits are those of the same MV on every job
    assert np.array_equal(exp["bits"], res["bits"])
    # and the search's own pick is never dearer than the golden's frac_cost says
    assert np.array_equal(surface.regret(res, surf)["search_cost"], res["frac_cost"])
    # the direct cost differs from the shipped one somewhere: the mode is not a no-op
    assert (exp["frac_cost"] != res["frac_cost"]).any() and (exp["cost"] != res["cost"]).any()


def test_tail_numpy_weights_and_wraps():
    job = np.zeros(1, surface.JOB_DTYPE)[0]
    job["mvp_x"], job["mvp_y"], job["bits_in"] = 3, -2, 7
    ml = 65536.0 * 4.0
    mvb = surface._eg_bits(10 - 3) + surface._eg_bits(-5 + 2)
    cost, bits = direct.tail_numpy(1000, 10, -5, job, ml)
    assert bits == 7 + mvb and cost == (1000 - 4 * mvb) + 4 * bits
    job["flags"] = JOB_BIPRED
    cost, _ = direct.tail_numpy(1001, 10, -5, job, ml)
    assert cost == (1001 - 4 * mvb) // 2 + 4 * bits            # floor of the halved difference
    cost, _ = direct.tail_numpy(0, 10, -5, job, ml)               # frac_cost below the MV cost: negative
    assert cost == ((-(4 * mvb)) // 2 + 4 * bits) & 0xFFFFFFFF    # floor, then the (UInt)(Int64) conversion
    job["flags"] = 0
    job["bits_in"] = 0
    cost, _ = direct.tail_numpy(0, 10, -5, job, 65536.0 * 1000.0)
    assert cost == 0 and (-(1000 * mvb) + 1000 * mvb) == 0
    cost, _ = direct.tail_numpy(5, 10, -5, job, 65536.0 * 1000.0)
    assert cost == 5
    job["flags"] = JOB_BIPRED
    cost, _ = direct.tail_numpy(5, 10, -5, job, 65536.0 * 1000.0)
    want = (5 - 1000 * mvb) // 2 + 1000 * mvb
    assert cost == want & 0xFFFFFFFF


def test_direct_numpy_refuses_records_without_a_class():
    g, idx, surf = subset(FIXTURES[0])
    res = g["results"][idx].copy()
    res["nn_class"][3] = 255
    with pytest.raises(ValueError):
        direct.direct_numpy(g["jobs"][idx], res, surf, g["lambdas"])
