"""Candidate-set refinement on the GPU (include/fme_among.h, csrc/fme_among.hip): fme_refine_among*
against nnfme.among.among_numpy on every fixture of the direct tests, with seeded lists that put every
class into every slot, empties, duplicates and lists of one, in every form; ties on flat and two-level
content; jobs refused one by one and batches rejected whole; fme_nn_rank_device against rank_numpy and
against crafted weights; fme_refine_topk* against fme_refine_direct, topk_numpy, batch splits and the
ordinary run's state; all kinds interleaved on two streams; bound planes; the C++ adapter; and
predictor.run(topk=).  Every comparison is == on integers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_bit_depth, load_golden
from nnfme import among, direct, predictor, surface, weights
from nnfme.abi import (E_INVALID, E_STATE, E_UNSUPPORTED, JOB_DTYPE, JOB_LOSSLESS, MV_RESULT_DTYPE, RES_REJECTED,
                       RESULT_DTYPE, compare_results)
from nnfme.predictor import NN_ROW_DTYPE
from nnfme.runtime import FmeContext, FmeError
from test_direct_numpy import FIXTURES, NN_GOLDENS, subset
from test_gpu_direct import _close, _host, _open, _records, _same, _upload, expected
from test_stress_oracle import LAMBDAS, refine_case, setup

pytestmark = pytest.mark.gpu

EMPTY = among.AMONG_EMPTY
RANK_FIXTURES = ("ldp_qp22_hadme_fen1_nn", "fen3_qp27_nn", "qp32_nn", "qp37_nn", "main10_fen3_qp27_nn")


def _blank(n, dtype=RESULT_DTYPE):
    out = np.zeros(n, dtype)
    out["status"] = RES_REJECTED
    return out


def _params(name):
    return weights.load_weights(int(load_golden(name)["config"][3]))


def _cand_dev(cand):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cand, dtype=np.uint8)).cuda()


def _among_dev(ctx, d_jobs, d_rows, cand, mv=False, costs=True):
    """One device among batch over host lists: (records, cand_cost or None)."""
    import torch
    n, k = cand.shape
    d_cand = _cand_dev(cand)
    dt = MV_RESULT_DTYPE if mv else RESULT_DTYPE
    d_out = _records(n, dt)
    d_cost = torch.full((n * k,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if costs else None
    (among.refine_among_mv_device if mv else among.refine_among_device)(ctx, d_jobs, d_rows, d_cand, k, d_out, d_cost, n)
    assert ctx.refine_status() == 0
    return _host(d_out, dt), (d_cost.cpu().numpy().view(np.uint32).reshape(n, k) if costs else None)


def seeded_lists(n, seed):
    """uint8 [n, 8] (n >= 500): rows 0..9 hold empties at the front, in the middle and at the end, lists
    of one, duplicates; below them every class occurs in every slot."""
    assert n >= 500
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 49, (n, 8)).astype(np.uint8)
    c[0, 0] = EMPTY
    c[1, :2] = EMPTY
    c[2, 3:5] = EMPTY
    c[3, 7] = EMPTY
    c[4, 5:] = EMPTY
    c[5, 1:] = EMPTY                        # lists of one: in slot 0, 7 and 3
    c[6, :7] = EMPTY
    c[7] = EMPTY
    c[7, 3] = 17
    c[8] = [5, 5, 40, 40, 5, 24, 24, 40]    # duplicates
    c[9] = 31                               # one class eight times
    for s in range(8):
        c[10 + rng.permutation(n - 10)[:49], s] = np.arange(49)
    for s in range(8):
        assert set(c[:, s].tolist()) >= set(range(49)), s
    return c


def _gathered(surf, cand):
    cost = surface._cost_rows(surf)
    on = cand != EMPTY
    return np.where(on, cost[np.arange(len(cand))[:, None], np.where(on, cand, 0)], among.NONE).astype(np.uint32)


# ---- 1. every fixture, every form ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_among_equals_among_numpy(name):
    _, _, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    reps = -(-500 // n)
    N = reps * n
    cand = seeded_lists(N, 9100 + FIXTURES.index(name))
    tj, tref, tsurf = np.tile(jobs, reps), np.tile(ref, reps), np.tile(surf, reps)
    try:
        ctx.refine(jobs[:37])                                   # some state to leave alone
        st = ctx.nn_get_state()
        d_tj = _upload(tj)
        none, cc_none = _among_dev(ctx, d_tj, None, cand)
        assert among.refine_among_status(ctx) == 0
        assert np.array_equal(ctx.nn_get_state(), st)
        ctx.nn_reset()
        d_rows = _records(N, NN_ROW_DTYPE)
        predictor.nn_inputs_device(ctx, d_tj, d_rows, N)
        assert ctx.refine_status() == 0
        rows = _host(d_rows, NN_ROW_DTYPE)
        st = ctx.nn_get_state()
        with_rows, cc_rows = _among_dev(ctx, d_tj, d_rows, cand)
        mv, cc_mv = _among_dev(ctx, d_tj, d_rows, cand, mv=True)
        mv_none, _ = _among_dev(ctx, d_tj, None, cand, mv=True, costs=False)
        host, cc_host = among.refine_among(ctx, tj, cand, rows)
        host_none, cc_hn = among.refine_among(ctx, tj, cand)
        assert among.refine_among_status(ctx) == 0
        assert np.array_equal(ctx.nn_get_state(), st)           # neither read nor written
    finally:
        _close(ctx)
    want, want_cc = among.among_numpy(tj, tref, cand, tsurf, g["lambdas"])
    _same(none, want, name)
    assert none.tobytes() == with_rows.tobytes() == host.tobytes() == host_none.tobytes()
    assert mv.tobytes() == direct.mv_records(none).tobytes() == mv_none.tobytes()
    assert (none["status"] == among.AMONG_STATUS).all()
    # every slot's cost is the surface's at that slot's class: a wrong position in a slot that loses fails too
    assert np.array_equal(cc_none, _gathered(tsurf, cand)) and np.array_equal(cc_none, want_cc)
    for other in (cc_rows, cc_mv, cc_host, cc_hn):
        assert np.array_equal(other, cc_none)
    _, idx, s = subset(name)                                    # the surfaces restated in numpy
    sub, sub_cc = among.among_numpy(jobs[idx], ref[idx], cand[idx], s, g["lambdas"])
    _same(none[idx], sub, name + " subset")
    assert np.array_equal(cc_none[idx], sub_cc)
    assert ((jobs["flags"] & JOB_LOSSLESS) != 0).any() and (jobs["key_offset"] >= 0).any()
    assert len({(int(w), int(h)) for w, h in zip(jobs["w"], jobs["h"])}) == 24


# ---- 2. k = 1 is fme_refine_at; a repeated class -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ra_qp27_nn", "main10_ra_qp37_nn"])
def test_k1_is_refine_at_and_repeats_change_nothing(name):
    import torch
    _, _, ref, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cls = np.ascontiguousarray(ref["nn_class"]).astype(np.uint8)
    try:
        d_jobs = _upload(jobs)
        d_cls, d_at = torch.from_numpy(cls).cuda(), _records(n)
        predictor.refine_at_device(ctx, d_jobs, None, d_cls, d_at, n)
        at = _host(d_at)
        got = {k: _among_dev(ctx, d_jobs, None, np.repeat(cls[:, None], k, axis=1)) for k in range(1, 9)}
        assert ctx.refine_status() == 0 and among.refine_among_status(ctx) == 0
    finally:
        _close(ctx)
    want = at.copy()
    assert (at["status"] == among.AMONG_STATUS & ~among.RES_NN_AMONG).all()
    want["status"] |= among.RES_NN_AMONG
    for k in range(1, 9):
        _same(got[k][0], want, f"{name} k={k}")
        assert (got[k][1] == at["frac_cost"][:, None]).all()


# ---- 3. ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["flat", "twolevel"])
def test_the_first_slot_of_least_cost_wins(kind, bd):
    pics, jobs, keys = refine_case(kind, bd)
    jobs = jobs.copy()
    zero = LAMBDAS.index(0.0)
    jobs["lambda_id"][::2] = zero
    n = len(jobs)
    rng = np.random.default_rng(300 + bd)
    base = np.stack([rng.permutation(49)[:8] for _ in range(n)]).astype(np.uint8)
    ctx = FmeContext(bit_depth=bd, use_hadamard=1, nn_mode=1, qp=22, fast_inter_mode=1)
    try:
        setup(ctx, pics, keys)
        ref = ctx.refine(jobs)
        surf, _ = surface.cost_surface(ctx, surface.jobs_at_results(jobs, ref), pick=False)
        d_jobs = _upload(jobs)
        runs = []
        for seed in (0, 1, 2):
            cand = base[:, np.random.default_rng(seed).permutation(8)]
            runs.append((cand,) + _among_dev(ctx, d_jobs, None, cand))
    finally:
        ctx.close()
    cost = surface._cost_rows(surf)
    lam0 = jobs["lambda_id"] == zero
    tied = 0
    for cand, rec, cc in runs:
        assert np.array_equal(cc, _gathered(surf, cand))
        least = cc.min(axis=1)
        first = np.argmax(cc == least[:, None], axis=1)              # the first slot holding the least cost
        assert np.array_equal(rec["nn_class"], cand[np.arange(n), first]) and np.array_equal(rec["frac_cost"], least)
        tied += int(((cc == least[:, None]).sum(axis=1) > 1).sum())
        _same(rec, among.among_numpy(jobs, ref, cand, surf, LAMBDAS)[0], f"{kind} {bd}")
        if kind == "flat":                                           # lambda 0: all 49 costs equal, slot 0's class
            assert (cost[lam0] == cost[lam0][:, :1]).all()
            assert np.array_equal(rec["nn_class"][lam0], cand[lam0, 0])
    assert tied > 0 and lam0.sum() > 20


# ---- 4. refusals ---------------------------------------------------------------------------------------------------
def test_jobs_refused_one_by_one():
    name = "qp32_nn"
    _, _, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = 300
    jobs, ref, surf = jobs[:n], ref[:n], surf[:n]
    rng = np.random.default_rng(6)
    good = rng.integers(0, 49, (n, 8)).astype(np.uint8)
    good[::7, 2] = EMPTY
    cand = good.copy()
    cand[10, 5], cand[120, 0], cand[200, 7] = 49, 200, 254
    cand[250] = EMPTY
    try:
        d_jobs, d_rows = _upload(jobs), _records(n, NN_ROW_DTYPE)
        predictor.nn_inputs_device(ctx, d_jobs, d_rows, n)
        rows = _host(d_rows, NN_ROW_DTYPE)
        st = ctx.nn_get_state()
        base, base_cc = _among_dev(ctx, d_jobs, d_rows, good)
        assert among.refine_among_status(ctx) == 0
        bad_rows = rows.copy()
        bad_rows["mv_int_x"][77] = jobs["mv_x"][77] + 2         # two samples from the job's mv
        bad_rows["status"][78] |= RES_REJECTED                  # a row of a rejected inputs batch
        got, got_cc = _among_dev(ctx, d_jobs, _upload(bad_rows), cand)
        assert among.refine_among_status(ctx) == 6
        got_mv, mv_cc = _among_dev(ctx, d_jobs, _upload(bad_rows), cand, mv=True)
        assert among.refine_among_status(ctx) == 6
        none, none_cc = _among_dev(ctx, d_jobs, None, cand)     # without rows: the four lists
        assert among.refine_among_status(ctx) == 4
        assert np.array_equal(ctx.nn_get_state(), st)
        out = np.full(n, 0xA5, np.uint8).repeat(64).view(RESULT_DTYPE)
        for c, r in ((cand, None), (cand, rows), (good, bad_rows)):
            with pytest.raises(FmeError) as e:                  # the host form: nothing enqueued, nothing written
                among.refine_among(ctx, jobs, c, r, out=out)
            assert e.value.code == E_INVALID
        assert (out.view(np.uint8) == 0xA5).all()
        assert among.refine_among_status(ctx) == 4              # still the last batch's
        again, _ = _among_dev(ctx, d_jobs, d_rows, good)
        assert among.refine_among_status(ctx) == 0
    finally:
        _close(ctx)
    refused = np.zeros(n, bool)
    refused[[10, 77, 78, 120, 200, 250]] = True
    assert got[refused].tobytes() == _blank(6).tobytes() and (got_cc[refused] == among.NONE).all()
    assert got[~refused].tobytes() == base[~refused].tobytes() and np.array_equal(got_cc[~refused], base_cc[~refused])
    assert again.tobytes() == base.tobytes()
    assert got_mv.tobytes() == direct.mv_records(got).tobytes() and np.array_equal(mv_cc, got_cc)
    four = np.zeros(n, bool)
    four[[10, 120, 200, 250]] = True
    assert none[four].tobytes() == _blank(4).tobytes() and none[~four].tobytes() == base[~four].tobytes()
    assert (none_cc[four] == among.NONE).all() and np.array_equal(none_cc[~four], base_cc[~four])
    _same(base, among.among_numpy(jobs, ref, good, surf, g["lambdas"])[0], "valid lists")


@pytest.mark.parametrize("field,value", [("w", 20), ("key_offset", 10 ** 8)])
def test_an_invalid_job_rejects_the_whole_batch(field, value):
    import torch
    name = "qp32_nn"
    g, ctx, jobs, keep = _open(name)
    a, b = 200, 400
    bad = jobs[a:b].copy()
    bad[field][17] = value
    n = b - a
    cand = np.random.default_rng(3).integers(0, 49, (n, 8)).astype(np.uint8)
    try:
        first = ctx.refine(jobs[:a])
        st = ctx.nn_get_state()
        d_bad, d_cand = _upload(bad), _cand_dev(cand)
        good_rows = _upload(predictor.rows_numpy(jobs[a:b], g["results"][a:b], st)[0])
        for rows in (None, good_rows):
            d_res, d_mv = _records(n), _records(n, MV_RESULT_DTYPE)
            d_cost = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
            among.refine_among_device(ctx, d_bad, rows, d_cand, 8, d_res, d_cost, n)
            assert ctx.refine_status() == 1 and among.refine_among_status(ctx) == 0
            assert _host(d_res).tobytes() == _blank(n).tobytes()
            assert (d_cost.cpu().numpy().view(np.uint32) == among.NONE).all()
            among.refine_among_mv_device(ctx, d_bad, rows, d_cand, 8, d_mv, None, n)
            assert ctx.refine_status() == 1
            assert _host(d_mv, MV_RESULT_DTYPE).tobytes() == _blank(n, MV_RESULT_DTYPE).tobytes()
        d_res = _records(n)
        among.refine_topk_device(ctx, d_bad, d_res, 4, None, None, n)     # the top-K batch likewise
        assert ctx.refine_status() == 1 and _host(d_res).tobytes() == _blank(n).tobytes()
        for call in (lambda: among.refine_among(ctx, bad, cand), lambda: among.refine_topk(ctx, bad, 4)):
            with pytest.raises(FmeError) as e:                  # the host forms: FME_E_INVALID
                call()
            assert e.value.code == E_INVALID
        assert np.array_equal(ctx.nn_get_state(), st)
        rest = ctx.refine(jobs[a:])                             # the context stays usable
        assert ctx.refine_status() == 0
    finally:
        _close(ctx)
    assert compare_results(np.concatenate([first, rest]), g["results"])[0] == 0


def test_bound_nn_rows_request_checks_and_timings():
    import torch
    g, ctx, jobs, keep = _open("qp37_nn")
    n = 64
    try:
        lib = among.bind(ctx.lib)
        res0, cc0 = among.refine_among(ctx, jobs[:0], np.zeros((0, 8), np.uint8))
        assert len(res0) == 0 and cc0.shape == (0, 8)
        assert lib.fme_refine_among_device(ctx.h, None, None, None, 8, None, None, 0, None) == 0
        assert lib.fme_refine_topk_device(ctx.h, None, None, 8, None, None, 0, None) == 0
        assert lib.fme_nn_rank_device(ctx.h, None, None, 8, 0, None) == 0
        assert lib.fme_refine_among_device(ctx.h, None, None, None, 8, None, None, 4, None) == E_INVALID
        assert among.refine_among_status(ctx) == 0              # before the first batch
        with pytest.raises(FmeError) as e:
            among.last_ms(ctx)                                  # no profiled call yet
        assert e.value.code == E_STATE
        d_jobs, d_rows, d_res = _upload(jobs[:n]), _records(n, NN_ROW_DTYPE), _records(n)
        d_cand = torch.full((n * 8,), 24, dtype=torch.uint8, device="cuda")
        for k in (0, 9):
            assert lib.fme_refine_among_device(ctx.h, d_jobs.data_ptr(), None, d_cand.data_ptr(), k, d_res.data_ptr(), None,
                                               n, None) == E_INVALID
            assert lib.fme_refine_topk_device(ctx.h, d_jobs.data_ptr(), d_res.data_ptr(), k, None, None, n, None) == E_INVALID
        bound = torch.zeros(9 * n, dtype=torch.int32, device="cuda")
        st = ctx.nn_get_state()
        ctx.set_nn_inputs(bound.data_ptr(), n)
        calls = (lambda: among.refine_among(ctx, jobs[:n], np.full((n, 8), 24, np.uint8)),
                 lambda: among.refine_among_device(ctx, d_jobs, None, d_cand, 8, d_res, None, n),
                 lambda: among.refine_among_mv_device(ctx, d_jobs, None, d_cand, 8, d_res, None, n),
                 lambda: among.refine_topk(ctx, jobs[:n], 4),
                 lambda: among.refine_topk_device(ctx, d_jobs, d_res, 4, None, None, n),
                 lambda: among.refine_topk_mv_device(ctx, d_jobs, d_res, 4, None, None, n))
        for call in calls:
            with pytest.raises(FmeError) as e:
                call()
            assert e.value.code == E_STATE
        ctx.set_nn_inputs(None)
        assert (_host(d_res, np.dtype("u1")) == 0xA5).all() and np.array_equal(ctx.nn_get_state(), st)
        ctx.set_profiling(True)
        among.refine_among_device(ctx, d_jobs, None, d_cand, 8, d_res, None, n)
        ms = among.last_ms(ctx)
        assert ms["emi"] > 0 and ms["rows"] == 0 and ms["rank"] == 0 and 0 < ms["evaluation"] <= ms["batch"] + 1e-3
        predictor.nn_inputs_device(ctx, d_jobs, d_rows, n)
        among.refine_among_device(ctx, d_jobs, d_rows, d_cand, 8, d_res, None, n)
        ms = among.last_ms(ctx)
        assert ms["emi"] == 0 and ms["rows"] == 0 and ms["rank"] == 0 and ms["evaluation"] > 0
        among.nn_rank_device(ctx, d_rows, d_cand, 8, n)
        ms = among.last_ms(ctx)
        assert ms["rank"] > 0 and ms["evaluation"] == 0 and ms["emi"] == 0
        among.refine_topk_device(ctx, d_jobs, d_res, 4, None, None, n)
        ms = among.last_ms(ctx)
        assert all(ms[p] > 0 for p in among.LAST_MS_NAMES)
        assert ms["batch"] >= ms["emi"] + ms["rows"] + ms["rank"] + ms["evaluation"] - 1e-3
    finally:
        _close(ctx)


# ---- 5. the ranking ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_rows(name):
    """(rows fme_nn_inputs gives for the fixture from a reset state, restated in numpy; read only)."""
    _, _, ref, _ = expected(name)
    rows, _ = predictor.rows_numpy(load_golden(name)["jobs"], ref, None)
    rows.setflags(write=False)
    return rows


def _rank_dev(ctx, d_rows, k, n, pad=64, offset=0):
    """fme_nn_rank_device into a poisoned buffer of n*k + pad bytes, `offset` bytes in: (cand, the bytes
    around them)."""
    import torch
    buf = torch.full((offset + n * k + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    among.nn_rank_device(ctx, d_rows, buf.data_ptr() + offset, k, n)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[offset:offset + n * k].reshape(n, k), np.r_[h[:offset], h[offset + n * k:]]


@pytest.mark.parametrize("name", RANK_FIXTURES)
def test_rank_equals_rank_numpy(name):
    _, _, ref, _ = expected(name)
    rows = _fixture_rows(name)
    params = _params(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    try:
        d_rows = _records(n, NN_ROW_DTYPE)
        predictor.nn_inputs_device(ctx, _upload(jobs), d_rows, n)
        assert ctx.refine_status() == 0
        _same(_host(d_rows, NN_ROW_DTYPE), rows, name + " rows")
        st = ctx.nn_get_state()
        got = {k: _rank_dev(ctx, d_rows, k, n) for k in (1, 3, 8)}
        assert np.array_equal(ctx.nn_get_state(), st)
    finally:
        _close(ctx)
    want = among.rank_numpy(params, rows, 8)
    for k, (cand, around) in got.items():
        assert np.array_equal(cand, want[:, :k]), (name, k)
        assert (around == 0xA5).all()
    top = got[8][0]
    assert np.array_equal(top[:, 0], ref["nn_class"])          # the class fme_refine records for the same inputs
    assert all(len(set(r.tolist())) == 8 for r in top) and top.max() < 49


def test_rank_ties_rejected_rows_odd_sizes_and_modes():
    name = "fen3_qp27_nn"
    rows = _fixture_rows(name)
    params = _params(name)
    g, ctx, jobs, keep = _open(name)
    off = FmeContext(use_hadamard=1, nn_mode=0, qp=22, fast_inter_mode=1)
    g2, deep, _, keep2 = _open("deep_master_qp22")
    n = 77                                                      # no multiple of 64; n*3 no multiple of 8
    try:
        bad = rows[:n].copy()
        bad["status"][5] = RES_REJECTED
        bad["status"][70] |= RES_REJECTED
        d_rows = _upload(bad)
        want = among.rank_numpy(params, bad, 8)
        for k, offset in ((3, 0), (3, 1), (8, 0), (8, 4), (8, 3), (5, 0), (1, 0)):
            cand, around = _rank_dev(ctx, d_rows, k, n, offset=offset)
            assert np.array_equal(cand, want[:, :k]), (k, offset)
            assert (around == 0xA5).all(), (k, offset)          # nothing beyond the n*k bytes
        assert (want[5] == EMPTY).all() and (want[70] == EMPTY).all() and (want[6] != EMPTY).all()
        t = weights.unpack(params.copy())
        t["h2_out"][:] = 0                                      # the output layer zero with equal biases
        t["bout"][:] = 0.25
        ctx.load_nn(weights.pack(t))
        cand, _ = _rank_dev(ctx, _upload(rows[:n]), 8, n)
        assert (cand == np.arange(8, dtype=np.uint8)[None, :]).all()
        t["bout"][:] = np.arange(49, dtype=np.float32)          # strictly increasing with the class
        ctx.load_nn(weights.pack(t))
        cand, _ = _rank_dev(ctx, _upload(rows[:n]), 8, n)
        assert (cand == (48 - np.arange(8, dtype=np.uint8))[None, :]).all()
        d_cand = _cand_dev(np.full((n, 8), 0xA5, np.uint8))
        for c, code in ((off, E_STATE), (deep, E_UNSUPPORTED)):
            with pytest.raises(FmeError) as e:
                among.nn_rank_device(c, d_rows, d_cand, 8, n)
            assert e.value.code == code
            with pytest.raises(FmeError) as e:
                among.refine_topk_device(c, _upload(jobs[:n]), _records(n), 4, None, None, n)
            assert e.value.code == code
        assert (d_cand.cpu().numpy() == 0xA5).all()
    finally:
        off.close()
        _close(deep)
        _close(ctx)


# ---- 6. top-K ------------------------------------------------------------------------------------------------------
def _topk_dev(ctx, d_jobs, k, n, mv=False, cand=True):
    import torch
    dt = MV_RESULT_DTYPE if mv else RESULT_DTYPE
    d_out = _records(n, dt)
    d_cand = torch.full((n * k,), 0xA5, dtype=torch.uint8, device="cuda") if cand else None
    d_cost = torch.zeros(n * k, dtype=torch.int32, device="cuda")
    (among.refine_topk_mv_device if mv else among.refine_topk_device)(ctx, d_jobs, d_out, k, d_cand, d_cost, n)
    assert ctx.refine_status() == 0 and among.refine_among_status(ctx) == 0
    return (_host(d_out, dt), d_cand.cpu().numpy().reshape(n, k) if cand else None,
            d_cost.cpu().numpy().view(np.uint32).reshape(n, k))


@pytest.mark.parametrize("name", ["fen3_qp27_nn", "main10_ldp_qp22_hadme_fen1_nn"])
def test_topk_against_direct_topk_numpy_and_splits(name):
    import torch
    exp, state, ref, surf = expected(name)
    params = _params(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cuts = sorted(int(v) for v in np.random.default_rng(44).integers(1, n, 3))
    try:
        d_jobs = _upload(jobs)
        got = {}
        for k in (1, 4, 8):
            ctx.nn_reset()
            got[k] = _topk_dev(ctx, d_jobs, k, n)
            assert np.array_equal(ctx.nn_get_state(), state), k   # what fme_refine_direct leaves
        ctx.nn_reset()
        mv4 = _topk_dev(ctx, d_jobs, 4, n, mv=True, cand=False)
        ctx.nn_reset()
        host4 = among.refine_topk(ctx, jobs, 4)
        assert np.array_equal(ctx.nn_get_state(), state)
        pieces = {}
        for cut in cuts:
            ctx.nn_reset()
            d_res = _records(n)
            d_cand = torch.full((n * 4,), 0xA5, dtype=torch.uint8, device="cuda")
            for a, b in ((0, cut), (cut, n)):
                among.refine_topk_device(ctx, d_jobs.data_ptr() + a * JOB_DTYPE.itemsize, d_res.data_ptr() + 64 * a, 4,
                                         d_cand.data_ptr() + 4 * a, None, b - a)
            assert ctx.refine_status() == 0 and among.refine_among_status(ctx) == 0
            pieces[cut] = (_host(d_res), d_cand.cpu().numpy().reshape(n, 4), ctx.nn_get_state())
    finally:
        _close(ctx)
    one = exp.copy()                                            # k = 1: fme_refine_direct's records, one more bit
    one["status"] |= among.RES_NN_AMONG
    _same(got[1][0], one, name + " k=1")
    assert np.array_equal(got[1][1][:, 0], ref["nn_class"])
    want, want_cand, want_cc, want_state = among.topk_numpy(jobs, ref, params, 4, surf, g["lambdas"])
    _same(got[4][0], want, name + " k=4")
    assert np.array_equal(got[4][1], want_cand) and np.array_equal(got[4][2], want_cc) and np.array_equal(want_state, state)
    rows, _ = predictor.rows_numpy(jobs, ref, None)
    for k in (1, 4, 8):
        assert np.array_equal(got[k][1], among.rank_numpy(params, rows, k)), k
        assert (got[k][0]["status"] & (predictor.RES_NN_EXTERN | among.TOPK_STATUS) == among.TOPK_STATUS).all()
    assert np.array_equal(got[4][0]["status"] & 3, ref["status"] & 3) and (ref["status"] & 3).any()
    assert (got[8][0]["frac_cost"] <= got[4][0]["frac_cost"]).all() and (got[4][0]["frac_cost"] <= got[1][0]["frac_cost"]).all()
    assert (got[8][0]["frac_cost"] < got[1][0]["frac_cost"]).any()
    assert mv4[0].tobytes() == direct.mv_records(got[4][0]).tobytes() and np.array_equal(mv4[2], got[4][2])
    assert host4[0].tobytes() == got[4][0].tobytes() and np.array_equal(host4[1], got[4][1]) and np.array_equal(host4[2], got[4][2])
    for cut, (r, c, st) in pieces.items():
        assert r.tobytes() == got[4][0].tobytes() and np.array_equal(c, got[4][1]) and np.array_equal(st, state), cut


# ---- 7. interleaved with the other kinds on two streams --------------------------------------------------------------
@pytest.mark.parametrize("reject", [False, True], ids=["valid", "among_rejected"])
@pytest.mark.parametrize("name", ["ldp_qp22_hadme_fen1_nn", "main10_fen3_qp27_nn"])
def test_interleaved_with_the_other_kinds(name, reject):
    import torch
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    rng = np.random.default_rng(12)
    cuts = [0, *sorted(int(v) for v in rng.choice(np.arange(64, n - 64), 4, replace=False)), n]
    parts = [jobs[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    if reject:
        parts[3]["w"][5] = 20
    cand = rng.integers(0, 49, (len(parts[3]), 4)).astype(np.uint8)

    def enqueue(sa, sb):
        """ordinary, top-K, direct, among, ordinary: (device outputs, the state copied behind them)."""
        d_jobs = [_upload(p) for p in parts]
        d_res = [_records(len(p)) for p in parts]
        d_cand, d_state = _cand_dev(cand), torch.zeros(12, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        a = None if sa is None else sa.cuda_stream
        b = None if sb is None else sb.cuda_stream
        sync = (lambda: torch.cuda.synchronize()) if sa is None else (lambda: None)
        ctx.refine_device(d_jobs[0].data_ptr(), d_res[0].data_ptr(), len(parts[0]), a)
        sync()
        among.refine_topk_device(ctx, d_jobs[1], d_res[1], 3, None, None, len(parts[1]), b)
        sync()
        direct.refine_direct_device(ctx, d_jobs[2], d_res[2], len(parts[2]), a)
        sync()
        among.refine_among_device(ctx, d_jobs[3], None, d_cand, 4, d_res[3], None, len(parts[3]), b)
        sync()
        ctx.refine_device(d_jobs[4].data_ptr(), d_res[4].data_ptr(), len(parts[4]), a)
        ctx.nn_copy_state_device(d_state.data_ptr(), a)
        assert ctx.refine_status() == 0
        torch.cuda.synchronize()
        return [_host(t) for t in d_res], d_state.cpu().numpy().view(np.uint32), ctx.nn_get_state()

    try:
        serial, serial_dev, serial_state = enqueue(None, None)   # one by one, the host waiting after each
        ctx.nn_reset()
        got, dev_state, state = enqueue(torch.cuda.Stream(), torch.cuda.Stream())
    finally:
        _close(ctx)
    for k in range(5):
        _same(got[k], serial[k], f"{name} batch {k}")
    assert np.array_equal(state, serial_state) and np.array_equal(dev_state, state) and np.array_equal(serial_dev, state)
    if reject:
        assert got[3].tobytes() == _blank(len(parts[3])).tobytes()
    else:
        assert (got[3]["status"] == among.AMONG_STATUS).all()
    # ordinary, top-K and direct batches carry the classes of one uninterrupted ordinary run (the among
    # batch leaves the state alone, so the batch after it does not see its jobs)
    assert compare_results(got[0], g["results"][:cuts[1]])[0] == 0
    assert np.array_equal(got[2]["nn_class"], g["results"]["nn_class"][cuts[2]:cuts[3]])
    assert (got[1]["status"] & among.TOPK_STATUS == among.TOPK_STATUS).all()


# ---- 8. bound planes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fen3_qp27_nn", "main10_fen3_qp27_nn"])
def test_bound_planes_with_odd_pitch(name):
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cand = np.random.default_rng(81).integers(0, 49, (n, 8)).astype(np.uint8)
    try:
        plain, plain_cc = _among_dev(ctx, _upload(jobs), None, cand)
    finally:
        _close(ctx)
    g, ctx, jobs, keep = _open(name, bind="C")
    try:
        bound, bound_cc = _among_dev(ctx, _upload(jobs), None, cand)
        assert among.refine_among_status(ctx) == 0
    finally:
        _close(ctx)
    _same(bound, plain, name + " geometry C")
    assert np.array_equal(bound_cc, plain_cc)


# ---- 9. the C++ adapter ----------------------------------------------------------------------------------------------
def test_cpp_topk_adapter(tmp_path):
    """fme_hm::CtuRowBatcher and FracSearch::refine with SearchConfig::nnTopK = 4 (include/fme_hm.hpp) on a
    fixture exported as raw arrays, through tests/cpp/test_topk_adapter.cpp compiled here against the built
    libraries: byte-equal records to the Python path's."""
    name = "ldp_qp22_hadme_fen1_nn"
    pkg = os.path.join(ROOT, "hm16.9-nn_fme_amd")
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "test_topk_adapter")
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "test_topk_adapter.cpp"), "-L", pkg, "-lfme_hm", "-lfme_amd",
                        f"-Wl,-rpath,{pkg}", "-lpthread", "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    g, ctx, jobs, keep = _open(name)
    try:
        exp, _, _ = among.refine_topk(ctx, jobs, 4)
    finally:
        _close(ctx)
    bd = golden_bit_depth(g)
    n = len(jobs)
    np.ascontiguousarray(g["pictures"], dtype=np.uint16 if bd > 8 else np.uint8).tofile(tmp_path / "pictures.raw")
    np.ascontiguousarray(g["keys"], dtype=np.int16).tofile(tmp_path / "keys.raw")
    np.ascontiguousarray(g["lambdas"], dtype=np.float64).tofile(tmp_path / "lambdas.raw")
    np.ascontiguousarray(jobs).tofile(tmp_path / "jobs.raw")
    np.ascontiguousarray(exp).tofile(tmp_path / "expected.raw")
    (tmp_path / "meta.txt").write_text(f"{g['pictures'].shape[2]} {g['pictures'].shape[1]} {g['pictures'].shape[0]} {n} "
                                       f"{len(g['keys'])} {len(g['lambdas'])}\n")
    hadme, fen, _, qp = (int(v) for v in g["config"][:4])
    p = subprocess.run([exe, str(tmp_path), str(bd), str(hadme), str(fen), str(qp), "4"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "topk adapter ok" in p.stdout


# ---- 10. a torch predictor's short list ----------------------------------------------------------------------------
def test_predictor_run_with_topk():
    import torch

    class Model(torch.nn.Module):
        takes_rows = True                       # integer arithmetic only: the rows' words, not float features

        def forward(self, w):
            u = w.to(torch.int64) & 0xFFFFFFFF
            first = (u[:, 8] + u[:, 9] + u[:, 0]) % 49
            score = -((torch.arange(49, device=w.device)[None, :] - first[:, None]) % 49)   # first, first + 1, ...
            return score.to(torch.float32)

    name = "fen3_qp27_nn"
    _, state, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cuts = [0, 3, 130, n]
    parts = list(zip(cuts[:-1], cuts[1:]))
    try:
        model = Model()
        d_jobs = [_upload(jobs[a:b]) for a, b in parts]
        d_rows = [_records(b - a, NN_ROW_DTYPE) for a, b in parts]
        d_res = [_records(b - a) for a, b in parts]
        d_cls = [torch.full(((b - a) * 3,), 0xA5, dtype=torch.uint8, device="cuda") for a, b in parts]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k in range(len(parts)):             # back to back, nothing waits in between
            predictor.run(ctx, d_jobs[k], model, d_rows[k], d_cls[k], d_res[k], s, topk=3)
        s.synchronize()
        assert ctx.refine_status() == 0 and among.refine_among_status(ctx) == 0
        rows = np.concatenate([_host(t, NN_ROW_DTYPE) for t in d_rows])
        got = np.concatenate([_host(t) for t in d_res])
        cand = np.concatenate([t.cpu().numpy().reshape(-1, 3) for t in d_cls])
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    _same(rows, predictor.rows_numpy(jobs, ref, None)[0], "rows")
    first = (rows["c"].astype(np.int64) + rows["pu_h"] + rows["e"][:, 0]) % 49
    assert np.array_equal(cand, (first[:, None] + np.arange(3)[None, :]) % 49)
    _same(got, among.among_numpy(jobs, ref, cand, surf, g["lambdas"])[0], "records")
    assert np.array_equal(after, state)         # the state one fme_refine_direct would leave
