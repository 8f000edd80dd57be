"""The external predictor on the GPU (include/fme_extern.h, csrc/fme_extern.hip): fme_nn_inputs* against
nnfme.predictor.rows_numpy of the oracle's records at the NN tail's seams, interleaved with ordinary
batches and in every nn_mode; fme_refine_at* against refine_at_numpy on every fixture of the direct
tests, with the ordinary run's classes, with seeded classes that cover all 49, with and without rows;
jobs refused one by one and batches rejected whole; the compact records; batch splits; saturated
content; and predictor.run with a torch module between the two calls on one stream.
Every comparison is == on integers."""
import numpy as np
import pytest

from conftest import golden_bit_depth
from nnfme import direct, predictor, surface
from nnfme.abi import (E_INVALID, E_STATE, JOB_DTYPE, JOB_EMI, JOB_LOSSLESS, MV_RESULT_DTYPE, RES_REJECTED,
                       RESULT_DTYPE, compare_results)
from nnfme.predictor import NN_ROW_DTYPE
from nnfme.runtime import FmeContext, FmeError
import test_gpu_nn_tail as tail
from test_direct_numpy import FIXTURES, subset
from test_gpu_direct import _close, _host, _open, _records, _same, _upload, expected
from test_stress_oracle import LAMBDAS, hi_of, refine_case, setup

pytestmark = pytest.mark.gpu

AT_STATUS = direct.RES_NN_DIRECT | predictor.RES_NN_EXTERN


def _blank(n, dtype=RESULT_DTYPE):
    """n records of a refused job / a rejected batch: 0 but for the status."""
    out = np.zeros(n, dtype)
    out["status"] = RES_REJECTED
    return out


def _rows_dev(ctx, jobs, stream=None):
    """fme_nn_inputs_device over host jobs: (device jobs, device rows, the rows on the host)."""
    d_jobs, d_rows = _upload(jobs), _records(len(jobs), NN_ROW_DTYPE)
    predictor.nn_inputs_device(ctx, d_jobs, d_rows, len(jobs), stream)
    assert ctx.refine_status() == 0
    return d_jobs, d_rows, _host(d_rows, NN_ROW_DTYPE)


def _at_dev(ctx, d_jobs, d_rows, cls, n, mv=False):
    import torch
    d_cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).cuda()
    dt = MV_RESULT_DTYPE if mv else RESULT_DTYPE
    d_out = _records(n, dt)
    (predictor.refine_at_mv_device if mv else predictor.refine_at_device)(ctx, d_jobs, d_rows, d_cls, d_out, n)
    assert ctx.refine_status() == 0
    return _host(d_out, dt)


def _at_status(want):
    """`want` (direct_numpy's records) with fme_refine_at's status."""
    out = want.copy()
    out["status"] = AT_STATUS
    return out


# ---- 1. rows at the tail's seams --------------------------------------------------------------------------
_CTX = {}


def _seam_ctx():
    if "c" not in _CTX:
        _CTX["c"] = FmeContext(nn_mode=1, qp=22)
        tail._bind(_CTX["c"], 22)
    return _CTX["c"]


@pytest.mark.parametrize("n", tail.SIZES)
def test_rows_equal_the_oracles_across_seams(n):
    batches, want = tail._batches(n), tail._oracle(22, n)
    ctx = _seam_ctx()
    ctx.nn_reset()
    state = None
    for k, ((uj, _, _), (res, st)) in enumerate(zip(batches, want)):
        exp, state = predictor.rows_numpy(uj, res, state)
        assert np.array_equal(state, st)                      # rows_numpy's state is the oracle's
        _, _, got = _rows_dev(ctx, uj)
        _same(got, exp, f"n={n} batch {k}")
        assert np.array_equal(ctx.nn_get_state(), st), f"n={n} batch {k}: NN state"
    if n >= 64:
        first = want[0][0]
        emi = (batches[0][0]["flags"] & JOB_EMI) != 0
        assert (~emi).any() and (first["n_emi"][emi] < 8).any()


def test_rows_with_writers_many_waves_back():
    uj, _, _ = tail._stretch_jobs()
    tail._oracle(22, 1)                       # binds the QP 22 oracle
    o = tail._ORC[22]
    o.nn_reset()
    res, st = o.refine(uj), o.nn_get_state()
    assert (res["n_emi"][1000:2100] == 0).all()   # more than a whole scan block pushes nothing
    exp, state = predictor.rows_numpy(uj, res, None)
    ctx = _seam_ctx()
    ctx.nn_reset()
    _, _, got = _rows_dev(ctx, uj)
    _same(got, exp, "stretch")
    assert np.array_equal(state, st) and np.array_equal(ctx.nn_get_state(), st)


# ---- 2. interleaving with ordinary batches ------------------------------------------------------------------
def test_inputs_batch_then_ordinary_batch():
    name = "ldp_qp22_hadme_fen1_nn"
    _, state, ref, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    a = len(jobs) // 2 + 3
    try:
        _, _, rows = _rows_dev(ctx, jobs[:a])
        got_b = ctx.refine(jobs[a:])          # B after an inputs batch over A
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    # the second context of the comparison is expected()'s: fme_refine over A then B from a reset state
    _same(got_b, ref[a:], "B after an inputs batch")
    assert np.array_equal(after, state)
    exp_rows, _ = predictor.rows_numpy(jobs[:a], ref[:a], None)
    _same(rows, exp_rows, "A's rows")


@pytest.mark.parametrize("name", ["fen3_qp27_nn", "main10_fen3_qp27_nn"])
def test_inputs_batch_between_ordinary_batches_on_two_streams(name):
    import torch
    _, state, ref, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cuts = [0, n // 3, 2 * n // 3 + 5, n]
    parts = list(zip(cuts[:-1], cuts[1:]))
    try:
        d_jobs = [_upload(jobs[a:b]) for a, b in parts]
        d_res = [_records(b - a) for a, b in parts]
        d_rows = _records(parts[1][1] - parts[1][0], NN_ROW_DTYPE)
        d_state = torch.zeros(12, dtype=torch.int32, device="cuda")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.refine_device(d_jobs[0].data_ptr(), d_res[0].data_ptr(), parts[0][1] - parts[0][0], s1.cuda_stream)
        predictor.nn_inputs_device(ctx, d_jobs[1], d_rows, parts[1][1] - parts[1][0], s2.cuda_stream)
        ctx.refine_device(d_jobs[2].data_ptr(), d_res[2].data_ptr(), parts[2][1] - parts[2][0], s1.cuda_stream)
        ctx.nn_copy_state_device(d_state.data_ptr(), s1.cuda_stream)
        assert ctx.refine_status() == 0
        torch.cuda.synchronize()
        got0, got2, rows = _host(d_res[0]), _host(d_res[2]), _host(d_rows, NN_ROW_DTYPE)
        dev_state = d_state.cpu().numpy().view(np.uint32)
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    (a0, b0), (a1, b1), (a2, b2) = parts
    _same(got0, ref[a0:b0], name + " first")
    _same(got2, ref[a2:b2], name + " B")      # as after fme_refine over everything before it
    _, st1 = predictor.rows_numpy(jobs[a0:b0], ref[a0:b0], None)
    exp_rows, _ = predictor.rows_numpy(jobs[a1:b1], ref[a1:b1], st1)
    _same(rows, exp_rows, name + " rows")
    assert np.array_equal(after, state) and np.array_equal(dev_state, state)


# ---- 3. every nn_mode -------------------------------------------------------------------------------------------
def _open_as(name, variant):
    """The fixture's pictures, lambdas and keys in a context of nn_mode 0 ("off"), of the fixture's own
    configuration ("own"), or of the fixture's net with FME_NN_IN_SLOT_RESET ("slotreset")."""
    from conftest import load_golden
    from nnfme import weights
    g = load_golden(name)
    hadme, fen, nn_mode, qp = (int(v) for v in g["config"][:4])
    kw = dict(use_hadamard=hadme, nn_mode=0 if variant == "off" else nn_mode, qp=qp, fast_inter_mode=fen,
              bit_depth=golden_bit_depth(g))
    if "net" in g and variant != "off":
        kw["net"] = weights.case_net(str(g["net"]) + ("+slotreset" if variant == "slotreset" else ""))
    ctx = FmeContext(**kw)
    for i, p in enumerate(g["pictures"]):
        ctx.set_picture(i, p)
    for i, lam in enumerate(g["lambdas"]):
        ctx.set_lambda(i, float(lam))
    if g["keys"].size:
        ctx.set_keys(g["keys"])
    reset = variant == "slotreset"
    assert reset == bool("net" in kw and kw["net"].input_flags & weights.SLOT_RESET)
    return ctx, np.ascontiguousarray(g["jobs"]), reset


@pytest.mark.parametrize("name,variant", [("ldp_qp22_hadme_fen1_nn", "off"), ("ldp_qp22_hadme_fen1_nn", "own"),
                                          ("deep_master_qp22", "own"), ("deep_scr3x40_qp22", "slotreset")])
def test_rows_in_every_nn_mode(name, variant):
    ctx, jobs, reset = _open_as(name, variant)
    k = len(jobs) // 2 + 1
    try:
        ref = ctx.refine(jobs)                    # the context's own ordinary run: EMI fields, and the state it leaves
        state = ctx.nn_get_state()
        if variant == "off":
            assert (ref["nn_class"] == 255).all() and not state.any()   # nn_mode 0: no class, no state carried
        ctx.nn_reset()
        first = predictor.nn_inputs(ctx, jobs[:k])            # the host form, two chained batches
        mid = ctx.nn_get_state()
        second = predictor.nn_inputs(ctx, jobs[k:])
        after = ctx.nn_get_state()
    finally:
        ctx.close()
    exp, out = predictor.rows_numpy(jobs, ref, None, reset)
    _, st_mid = predictor.rows_numpy(jobs[:k], ref[:k], None, reset)
    _same(np.concatenate([first, second]), exp, f"{name} {variant}")
    assert np.array_equal(mid, st_mid) and np.array_equal(after, out)
    if variant != "off":
        assert np.array_equal(out, state)         # what fme_refine over the same jobs leaves
    else:                                         # the rule of nn_mode 1 all the same
        assert np.array_equal(out, expected(name)[1])
    own = np.where(np.arange(8)[None, :] < exp["n_emi"][:, None], ref["emi"], 0)
    assert (exp["e"] != own).any() != reset       # stale slots carried, or zeroed under the slot-reset rule
    if variant != "off":                          # the rows' status bits are the ordinary run's
        assert np.array_equal(exp["status"], ref["status"])


# ---- 4. fme_refine_at on every fixture ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_refine_at_equals_refine_at_numpy(name):
    exp, _, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    reps = -(-500 // n)
    rng = np.random.default_rng(8100 + FIXTURES.index(name))
    cls = rng.integers(0, 49, reps * n).astype(np.uint8)
    assert len(np.unique(cls)) == 49
    tj, tref, tsurf = np.tile(jobs, reps), np.tile(ref, reps), np.tile(surf, reps)
    try:
        ctx.refine(jobs[:37])                                  # some state to leave alone
        st = ctx.nn_get_state()
        d_jobs = _upload(jobs)
        own = _at_dev(ctx, d_jobs, None, ref["nn_class"], n)   # (a)
        d_tj = _upload(tj)
        rnd = _at_dev(ctx, d_tj, None, cls, reps * n)          # (b)
        assert predictor.refine_at_status(ctx) == 0
        assert np.array_equal(ctx.nn_get_state(), st)          # (d)
        ctx.nn_reset()
        _, d_rows, rows = _rows_dev(ctx, tj)                   # (c)
        st = ctx.nn_get_state()
        with_rows = _at_dev(ctx, d_tj, d_rows, cls, reps * n)
        host = predictor.refine_at(ctx, tj, cls, rows)         # the host form, with rows and without
        host_none = predictor.refine_at(ctx, tj, cls)
        assert predictor.refine_at_status(ctx) == 0
        assert np.array_equal(ctx.nn_get_state(), st)          # (d)
    finally:
        _close(ctx)
    _same(own, _at_status(exp), name + " own classes")
    want = predictor.refine_at_numpy(tj, tref, cls, tsurf, g["lambdas"])
    _same(rnd, want, name + " seeded classes")
    assert (rnd["nn_class"] == cls).all() and (rnd["status"] == AT_STATUS).all()
    assert with_rows.tobytes() == rnd.tobytes() == host.tobytes() == host_none.tobytes()
    _, idx, s = subset(name)                                   # the surfaces restated in numpy
    _same(rnd[idx], predictor.refine_at_numpy(jobs[idx], ref[idx], cls[idx], s, g["lambdas"]), name + " subset")
    assert ((jobs["flags"] & JOB_LOSSLESS) != 0).any() and (jobs["key_offset"] >= 0).any()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_jobs_refused_one_by_one():
    name = "qp32_nn"
    _, _, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = 300
    jobs, ref, surf = jobs[:n], ref[:n], surf[:n]
    rng = np.random.default_rng(5)
    good = rng.integers(0, 49, n).astype(np.uint8)
    cls = good.copy()
    cls[10], cls[200] = 49, 255
    try:
        d_jobs, d_rows, rows = _rows_dev(ctx, jobs)
        st = ctx.nn_get_state()
        base = _at_dev(ctx, d_jobs, d_rows, good, n)
        assert predictor.refine_at_status(ctx) == 0
        bad_rows = rows.copy()
        bad_rows["mv_int_x"][77] = jobs["mv_x"][77] + 2        # two samples from the job's mv
        ok_rows = rows.copy()                                  # one sample off is still the job's row
        ok_rows["mv_int_y"][78] = jobs["mv_y"][78] + (1 if rows["mv_int_y"][78] <= jobs["mv_y"][78] else -1)
        ok_rows["mv_int_x"][77] = bad_rows["mv_int_x"][77]
        got = _at_dev(ctx, d_jobs, _upload(ok_rows), cls, n)
        assert predictor.refine_at_status(ctx) == 3
        got_mv = _at_dev(ctx, d_jobs, _upload(ok_rows), cls, n, mv=True)
        assert predictor.refine_at_status(ctx) == 3
        none = _at_dev(ctx, d_jobs, None, cls, n)              # without rows: the two classes
        assert predictor.refine_at_status(ctx) == 2
        assert np.array_equal(ctx.nn_get_state(), st)
        out = np.full(n, 0xA5, np.uint8).repeat(64).view(RESULT_DTYPE)
        for c, r in ((cls, None), (cls, rows), (good, bad_rows)):
            with pytest.raises(FmeError) as e:                 # the host form: nothing enqueued, nothing written
                predictor.refine_at(ctx, jobs, c, r, out=out)
            assert e.value.code == E_INVALID
        assert (out.view(np.uint8) == 0xA5).all()
        assert predictor.refine_at_status(ctx) == 2            # still the last batch's
        again = _at_dev(ctx, d_jobs, d_rows, good, n)
        assert predictor.refine_at_status(ctx) == 0
    finally:
        _close(ctx)
    refused = np.zeros(n, bool)
    refused[[10, 77, 200]] = True
    assert got[refused].tobytes() == _blank(3).tobytes()
    moved = np.zeros(n, bool)
    moved[78] = ok_rows["mv_int_y"][78] != rows["mv_int_y"][78]
    keep_ = ~refused & ~moved
    assert got[keep_].tobytes() == base[keep_].tobytes() and again.tobytes() == base.tobytes()
    assert got["mv_int_y"][78] == ok_rows["mv_int_y"][78] and got["status"][78] == AT_STATUS
    assert got_mv.tobytes() == direct.mv_records(got).tobytes()
    two = np.zeros(n, bool)
    two[[10, 200]] = True
    assert none[two].tobytes() == _blank(2).tobytes() and none[~two].tobytes() == base[~two].tobytes()
    _same(base, predictor.refine_at_numpy(jobs, ref, good, surf, g["lambdas"]), "valid classes")


@pytest.mark.parametrize("field,value", [("w", 20), ("key_offset", 10 ** 8)])
def test_an_invalid_job_rejects_the_whole_batch(field, value):
    name = "qp32_nn"
    g, ctx, jobs, keep = _open(name)
    a, b = 200, 400
    bad = jobs[a:b].copy()
    bad[field][17] = value
    n = b - a
    cls = np.full(n, 24, np.uint8)
    try:
        first = ctx.refine(jobs[:a])
        st = ctx.nn_get_state()
        d_bad, d_rows = _upload(bad), _records(n, NN_ROW_DTYPE)
        predictor.nn_inputs_device(ctx, d_bad, d_rows, n)
        assert ctx.refine_status() == 1
        assert _host(d_rows, NN_ROW_DTYPE).tobytes() == _blank(n, NN_ROW_DTYPE).tobytes()
        assert np.array_equal(ctx.nn_get_state(), st)
        import torch
        d_cls = torch.from_numpy(cls).cuda()
        good_rows = _upload(predictor.rows_numpy(jobs[a:b], g["results"][a:b], st)[0])
        for rows in (None, good_rows):
            d_res, d_mv = _records(n), _records(n, MV_RESULT_DTYPE)
            predictor.refine_at_device(ctx, d_bad, rows, d_cls, d_res, n)
            assert ctx.refine_status() == 1 and predictor.refine_at_status(ctx) == 0
            assert _host(d_res).tobytes() == _blank(n).tobytes()
            predictor.refine_at_mv_device(ctx, d_bad, rows, d_cls, d_mv, n)
            assert ctx.refine_status() == 1
            assert _host(d_mv, MV_RESULT_DTYPE).tobytes() == _blank(n, MV_RESULT_DTYPE).tobytes()
        for call in (lambda: predictor.nn_inputs(ctx, bad), lambda: predictor.refine_at(ctx, bad, cls)):
            with pytest.raises(FmeError) as e:                 # the host forms: FME_E_INVALID
                call()
            assert e.value.code == E_INVALID
        assert np.array_equal(ctx.nn_get_state(), st)
        rest = ctx.refine(jobs[a:])                            # the next batch gives the fixture's results
        assert ctx.refine_status() == 0
    finally:
        _close(ctx)
    assert compare_results(np.concatenate([first, rest]), g["results"])[0] == 0


def test_bound_nn_rows_and_request_checks():
    import torch
    g, ctx, jobs, keep = _open("qp37_nn")
    n = 64
    try:
        lib = predictor.bind(ctx.lib)
        assert len(predictor.nn_inputs(ctx, jobs[:0])) == 0 and len(predictor.refine_at(ctx, jobs[:0], [])) == 0
        assert lib.fme_nn_inputs_device(ctx.h, None, None, 0, None) == 0
        assert lib.fme_refine_at_device(ctx.h, None, None, None, None, 0, None) == 0
        assert lib.fme_refine_at_mv_device(ctx.h, None, None, None, None, 0, None) == 0
        assert lib.fme_nn_inputs_device(ctx.h, None, None, 4, None) == E_INVALID
        assert predictor.refine_at_status(ctx) == 0            # before the first batch
        with pytest.raises(FmeError) as e:
            predictor.last_ms(ctx)                             # no profiled batch yet
        assert e.value.code == E_STATE
        bound = torch.zeros(9 * n, dtype=torch.int32, device="cuda")
        d_jobs, d_rows, d_res = _upload(jobs[:n]), _records(n, NN_ROW_DTYPE), _records(n)
        d_cls = torch.full((n,), 24, dtype=torch.uint8, device="cuda")
        st = ctx.nn_get_state()
        ctx.set_nn_inputs(bound.data_ptr(), n)
        calls = (lambda: predictor.nn_inputs(ctx, jobs[:n]), lambda: predictor.nn_inputs_device(ctx, d_jobs, d_rows, n),
                 lambda: predictor.refine_at(ctx, jobs[:n], np.full(n, 24, np.uint8)),
                 lambda: predictor.refine_at_device(ctx, d_jobs, None, d_cls, d_res, n),
                 lambda: predictor.refine_at_device(ctx, d_jobs, d_rows, d_cls, d_res, n),
                 lambda: predictor.refine_at_mv_device(ctx, d_jobs, None, d_cls, d_res, n))
        for call in calls:
            with pytest.raises(FmeError) as e:
                call()
            assert e.value.code == E_STATE
        ctx.set_nn_inputs(None)
        assert (_host(d_rows, np.dtype("u1")) == 0xA5).all() and (_host(d_res, np.dtype("u1")) == 0xA5).all()
        assert np.array_equal(ctx.nn_get_state(), st)
        ctx.set_profiling(True)
        predictor.nn_inputs_device(ctx, d_jobs, d_rows, n)
        ms = predictor.last_ms(ctx)
        assert ms["emi"] > 0 and ms["rows"] > 0 and ms["evaluation"] == 0 and ms["batch"] >= ms["emi"] + ms["rows"] - 1e-3
        predictor.refine_at_device(ctx, d_jobs, d_rows, d_cls, d_res, n)
        ms = predictor.last_ms(ctx)
        assert ms["emi"] == 0 and ms["rows"] == 0 and 0 < ms["evaluation"] <= ms["batch"] + 1e-3
        predictor.refine_at_device(ctx, d_jobs, None, d_cls, d_res, n)
        ms = predictor.last_ms(ctx)
        assert ms["emi"] > 0 and ms["rows"] == 0 and ms["evaluation"] > 0
    finally:
        _close(ctx)


# ---- 6. compact records and splits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ra_qp27_nn", "main10_ra_qp37_nn"])
def test_compact_records_and_split_batches(name):
    import torch
    _, _, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cls = np.random.default_rng(61).integers(0, 49, n).astype(np.uint8)
    try:
        d_jobs, d_rows, rows = _rows_dev(ctx, jobs)
        state = ctx.nn_get_state()
        full = _at_dev(ctx, d_jobs, d_rows, cls, n)
        mv_rows = _at_dev(ctx, d_jobs, d_rows, cls, n, mv=True)
        mv_none = _at_dev(ctx, d_jobs, None, cls, n, mv=True)
        d_cls = torch.from_numpy(cls).cuda()
        pieces = {}
        for cut in (1, 64, n - 1):
            ctx.nn_reset()
            d_r2, d_full, d_mv = _records(n, NN_ROW_DTYPE), _records(n), _records(n, MV_RESULT_DTYPE)
            for a, b in ((0, cut), (cut, n)):
                pj, pr, pc = d_jobs.data_ptr() + a * JOB_DTYPE.itemsize, d_r2.data_ptr() + 64 * a, d_cls.data_ptr() + a
                predictor.nn_inputs_device(ctx, pj, pr, b - a)
                predictor.refine_at_device(ctx, pj, pr, pc, d_full.data_ptr() + 64 * a, b - a)
                predictor.refine_at_mv_device(ctx, pj, None, pc, d_mv.data_ptr() + 16 * a, b - a)
            assert ctx.refine_status() == 0 and predictor.refine_at_status(ctx) == 0
            pieces[cut] = (_host(d_r2, NN_ROW_DTYPE), _host(d_full), _host(d_mv, MV_RESULT_DTYPE), ctx.nn_get_state())
    finally:
        _close(ctx)
    _same(full, predictor.refine_at_numpy(jobs, ref, cls, surf, g["lambdas"]), name)
    assert mv_rows.tobytes() == direct.mv_records(full).tobytes() == mv_none.tobytes()
    assert (mv_rows["reserved"] == 0).all()
    for cut, (r2, f2, m2, st2) in pieces.items():
        assert r2.tobytes() == rows.tobytes() and f2.tobytes() == full.tobytes() and m2.tobytes() == mv_rows.tobytes(), cut
        assert np.array_equal(st2, state), cut


# ---- 7. saturated content -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_saturated_pictures_and_extreme_keys(bd):
    pics, jobs, keys = refine_case("binary", bd)
    hi = hi_of(bd)
    assert int(keys.min()) == -hi and int(keys.max()) == 2 * hi
    cls = np.random.default_rng(70 + bd).integers(0, 49, len(jobs)).astype(np.uint8)
    ctx = FmeContext(bit_depth=bd, use_hadamard=1, nn_mode=1, qp=22, fast_inter_mode=1)
    try:
        setup(ctx, pics, keys)
        ref = ctx.refine(jobs)
        surf, _ = surface.cost_surface(ctx, surface.jobs_at_results(jobs, ref), pick=False)
        ctx.nn_reset()
        rows = predictor.nn_inputs(ctx, jobs)
        got = predictor.refine_at(ctx, jobs, cls)
        got_rows = predictor.refine_at(ctx, jobs, cls, rows)
    finally:
        ctx.close()
    _same(got, predictor.refine_at_numpy(jobs, ref, cls, surf, LAMBDAS), f"binary {bd}")
    assert got_rows.tobytes() == got.tobytes()
    _same(rows, predictor.rows_numpy(jobs, ref, None)[0], f"binary {bd} rows")


# ---- 8. a torch predictor between the two calls -------------------------------------------------------------------
def test_predictor_run_with_an_integer_torch_module():
    import torch

    class Model(torch.nn.Module):
        takes_rows = True                       # integer arithmetic only: the rows' words, not float features

        def forward(self, w):
            u = w.to(torch.int64) & 0xFFFFFFFF
            cls = (u[:, 8] + u[:, 9] + u[:, 0]) % 49
            return torch.nn.functional.one_hot(cls, 49)

    name = "fen3_qp27_nn"
    _, state, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    cuts = [0, 3, 130, n // 2, n]
    parts = list(zip(cuts[:-1], cuts[1:]))
    try:
        model = Model()
        d_jobs = [_upload(jobs[a:b]) for a, b in parts]
        d_rows = [_records(b - a, NN_ROW_DTYPE) for a, b in parts]
        d_res = [_records(b - a) for a, b in parts]
        d_cls = [torch.full((b - a,), 0xA5, dtype=torch.uint8, device="cuda") for a, b in parts]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k in range(len(parts)):             # back to back, nothing waits in between
            predictor.run(ctx, d_jobs[k], model, d_rows[k], d_cls[k], d_res[k], s)
        s.synchronize()
        assert ctx.refine_status() == 0 and predictor.refine_at_status(ctx) == 0
        rows = np.concatenate([_host(t, NN_ROW_DTYPE) for t in d_rows])
        got = np.concatenate([_host(t) for t in d_res])
        cls = np.concatenate([t.cpu().numpy() for t in d_cls])
        after = ctx.nn_get_state()
        feats = torch.cat([predictor.features_torch(t) for t in d_rows]).cpu().numpy()
    finally:
        _close(ctx)
    _same(rows, predictor.rows_numpy(jobs, ref, None)[0], "rows")
    want_cls = (rows["c"].astype(np.int64) + rows["pu_h"] + rows["e"][:, 0]) % 49
    assert np.array_equal(cls, want_cls) and len(np.unique(cls)) > 20
    _same(got, predictor.refine_at_numpy(jobs, ref, cls, surf, g["lambdas"]), "records")
    assert np.array_equal(after, state)         # the state one fme_refine_direct would leave
    assert feats.dtype == np.float32 and np.array_equal(feats, predictor.features(rows))
