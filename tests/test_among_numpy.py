"""Candidate-set refinement restated in numpy (nnfme.among) on a CPU, no library needed.

rank_numpy against the oracle: over rows built with predictor.rows_numpy from the NN goldens at the
four QPs its first slot is the golden nn_class and its full order is a stable descending sort of
orc_nn_forward's logits.  among_numpy against predictor.refine_at_numpy: k = 1 is that function apart
from the status bit, a permuted list changes the record only through ties, and where every cost ties
the chosen class is slot 0's.  Every comparison is == on integers."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from nnfme import among, predictor, surface, weights
from nnfme.abi import RES_REJECTED, RESULT_DTYPE
from oracle import Oracle
from test_direct_numpy import subset
from test_stress_oracle import LAMBDAS, refine_case, refine_expected

QP_GOLDENS = ("ldp_qp22_hadme_fen1_nn", "fen3_qp27_nn", "qp32_nn", "qp37_nn")
ROWS_PER_QP = 100


@functools.lru_cache(maxsize=None)
def golden_rows(name):
    """(params, rows of the fixture's first jobs from a reset state, the golden records of those jobs)."""
    g = load_golden(name)
    rows, _ = predictor.rows_numpy(g["jobs"], g["results"], None)
    return weights.load_weights(int(g["config"][3])), rows[:ROWS_PER_QP], g["results"][:ROWS_PER_QP]


def test_rank_numpy_is_the_oracles_order_at_the_four_qps():
    orc = Oracle()
    total = 0
    for name in QP_GOLDENS:
        params, rows, res = golden_rows(name)
        got = among.rank_numpy(params, rows, 8)
        assert got.shape == (len(rows), 8) and got.dtype == np.uint8
        assert np.array_equal(got[:, 0], res["nn_class"]), name
        logits = among.logits_numpy(params, rows)
        for i, r in enumerate(rows):
            cls, want = orc.nn_class(params, r["e"], r["c"], r["pu_h"], r["pu_w"])
            assert cls == res["nn_class"][i]
            assert logits[i].tobytes() == want.tobytes(), (name, i)       # bit-equal float32 outputs
            order = np.argsort(-want, kind="stable")
            assert np.array_equal(got[i], order[:8]), (name, i)
            assert len(set(got[i].tolist())) == 8
        for k in (1, 3):
            assert np.array_equal(among.rank_numpy(params, rows, k), got[:, :k])
        total += len(rows)
    assert total >= 300


def test_rank_numpy_ties_and_rejected_rows():
    params, rows, _ = golden_rows(QP_GOLDENS[0])
    t = weights.unpack(params.copy())
    t["h2_out"][:] = 0                    # the output layer zero with equal biases: every output ties
    t["bout"][:] = 0.25
    flat = among.rank_numpy(weights.pack(t), rows, 8)
    assert (flat == np.arange(8, dtype=np.uint8)[None, :]).all()
    t["bout"][:] = np.arange(49, dtype=np.float32)   # strictly increasing with the class
    up = among.rank_numpy(weights.pack(t), rows, 8)
    assert (up == (48 - np.arange(8, dtype=np.uint8))[None, :]).all()
    bad = rows.copy()
    bad["status"][5] = RES_REJECTED
    got = among.rank_numpy(params, bad, 3)
    assert (got[5] == among.AMONG_EMPTY).all() and np.array_equal(np.delete(got, 5, 0), np.delete(among.rank_numpy(params, rows, 3), 5, 0))
    assert np.array_equal(among.order_numpy(np.array([[1, 3, 3, 0, 3]], np.float32), 4), [[1, 2, 4, 0]])
    with pytest.raises(ValueError):
        among.rank_numpy(params, rows, 9)


@pytest.mark.parametrize("name", ["qp32_nn", "main10_fen3_qp27_nn"])
def test_among_numpy_against_refine_at_numpy(name):
    g, idx, surf = subset(name)
    jobs, res = g["jobs"][idx], g["results"][idx]
    n = len(jobs)
    rng = np.random.default_rng(31)
    cost = surface._cost_rows(surf)
    # k = 1: refine_at_numpy apart from the status bit
    cls = rng.integers(0, 49, n).astype(np.uint8)
    one, c1 = among.among_numpy(jobs, res, cls[:, None], surf, g["lambdas"])
    want = predictor.refine_at_numpy(jobs, res, cls, surf, g["lambdas"])
    assert np.array_equal(one["status"], want["status"] | among.RES_NN_AMONG)
    want["status"] |= among.RES_NN_AMONG
    assert one.tobytes() == want.tobytes() and np.array_equal(c1[:, 0], cost[np.arange(n), cls])
    # k = 8, distinct classes, one slot emptied: the least cost of the list, the first slot holding it
    lists = np.stack([rng.permutation(49)[:8] for _ in range(n)]).astype(np.uint8)
    lists[np.arange(n), rng.integers(0, 8, n)] = among.AMONG_EMPTY
    rec, cc = among.among_numpy(jobs, res, lists, surf, g["lambdas"])
    on = lists != among.AMONG_EMPTY
    gathered = np.where(on, cost[np.arange(n)[:, None], np.where(on, lists, 0)], among.NONE)
    assert np.array_equal(cc, gathered)
    least = np.where(on, gathered.astype(np.int64), 1 << 40).min(axis=1)
    assert np.array_equal(rec["frac_cost"], least) and (rec["status"] == among.AMONG_STATUS).all()
    for i in range(n):
        first = int(np.flatnonzero(on[i] & (gathered[i] == least[i]))[0])
        assert rec["nn_class"][i] == lists[i, first]
    # a permuted list: the costs move with the slots; the record changes only through ties
    moved = 0
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(8)
        rec2, cc2 = among.among_numpy(jobs, res, lists[:, perm], surf, g["lambdas"])
        assert np.array_equal(cc2, cc[:, perm]) and np.array_equal(rec2["frac_cost"], rec["frac_cost"])
        tied = (np.where(on, gathered.astype(np.int64), 1 << 40) == least[:, None]).sum(axis=1) > 1
        assert rec2[~tied].tobytes() == rec[~tied].tobytes()
        moved += int((rec2["nn_class"] != rec["nn_class"]).sum())
        assert ((rec2["nn_class"] != rec["nn_class"]) <= tied).all()
    # refusals: a slot in 49..254, no class at all
    bad = lists.copy()
    bad[0, 3], bad[1, 0], bad[2, 7] = 49, 200, 254
    bad[3] = among.AMONG_EMPTY
    rec3, cc3 = among.among_numpy(jobs, res, bad, surf, g["lambdas"])
    blank = np.zeros(4, RESULT_DTYPE)
    blank["status"] = RES_REJECTED
    assert rec3[:4].tobytes() == blank.tobytes() and (cc3[:4] == among.NONE).all()
    assert rec3[4:].tobytes() == rec[4:].tobytes() and np.array_equal(cc3[4:], cc[4:])
    assert np.array_equal(among.refused_lists(bad), np.arange(n) < 4)


def test_every_cost_ties_on_flat_content_so_slot_0_wins():
    pics, jobs, keys = refine_case("flat", 8)
    res, _ = refine_expected("flat", 8, 1)
    sel = np.flatnonzero((jobs["key_offset"] < 0) & (jobs["w"].astype(int) * jobs["h"] <= 256))[:24]
    assert len(sel) >= 12
    j = jobs[sel].copy()
    j["lambda_id"] = len(LAMBDAS) - 1
    assert LAMBDAS[-1] == 0.0
    surf = surface.surfaces_numpy(pics, keys, LAMBDAS, surface.jobs_at_results(j, res[sel]), 1, 8)
    cost = surface._cost_rows(surf)
    assert (cost == cost[:, :1]).all()                     # lambda 0 on a flat picture: all 49 costs equal
    rng = np.random.default_rng(9)
    lists = np.stack([rng.permutation(49)[:8] for _ in range(len(j))]).astype(np.uint8)
    for seed in (0, 1, 2):
        p = lists[:, np.random.default_rng(seed).permutation(8)]
        rec, cc = among.among_numpy(j, res[sel], p, surf, LAMBDAS)
        assert np.array_equal(rec["nn_class"], p[:, 0]) and (cc == cost[:, :1]).all()
    p = lists.copy()
    p[:, 0] = among.AMONG_EMPTY                            # an empty slot 0 is skipped: slot 1's class
    rec, _ = among.among_numpy(j, res[sel], p, surf, LAMBDAS)
    assert np.array_equal(rec["nn_class"], p[:, 1])
