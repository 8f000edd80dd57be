"""The external predictor's rows and records restated in numpy (nnfme.predictor) on a CPU, pinned to
the goldens: a row built from a golden's own records, fed to the net alone, must return the golden's
class for every job (so the row is what NN_pred() read); the state out must be the oracle's after
refining the same jobs; and with the golden's own classes refine_at_numpy is direct_numpy but for the
status.  Every comparison is == on integers."""
import functools
import os

import numpy as np
import pytest

from conftest import golden_bit_depth, load_golden
from nnfme import dataset, direct, predictor, weights
from nnfme.abi import JOB_EMI, RES_NN_STALE, RES_NN_UNINIT, RES_REJECTED, RESULT_DTYPE
from oracle import REF_SO, Oracle, Reference
from test_direct_numpy import FIXTURES, subset

HAVE_REF = os.path.exists(REF_SO)


def net_of(g):
    """The fixture's generic net (nn_mode 2), or None (the shipped weights of its QP)."""
    return weights.case_net(str(g["net"])) if "net" in g else None


def slot_reset_of(g):
    net = net_of(g)
    return bool(net is not None and net.input_flags & weights.SLOT_RESET)


@functools.lru_cache(maxsize=None)
def golden_rows(name):
    """(fixture, rows_numpy of its own records from a reset state, the state out), shared, read only."""
    g = load_golden(name)
    rows, out = predictor.rows_numpy(g["jobs"], g["results"], None, slot_reset_of(g))
    rows.setflags(write=False)
    out.setflags(write=False)
    return g, rows, out


def _engines(g):
    """The oracle (and the reference's own code where it is built) with the fixture's net loaded."""
    hadme, fen, nn_mode, qp = (int(v) for v in g["config"][:4])
    bd = golden_bit_depth(g)
    engines = [Oracle(use_hadamard=hadme, nn_mode=nn_mode, qp=qp, fast_inter_mode=fen, bit_depth=bd)]
    if HAVE_REF:
        engines.append(Reference(use_hadamard=hadme, nn_mode=nn_mode, fast_inter_mode=fen, bit_depth=bd))
    net = net_of(g)
    for e in engines:
        if net is not None:
            e.load_nn_net(net)
        else:
            e.load_nn(weights.load_weights(qp))
    return engines, net, qp


def test_row_dtype_is_the_header_struct():
    d = predictor.NN_ROW_DTYPE
    assert d.itemsize == 64
    off = {n: d.fields[n][1] for n in d.names}
    assert off == {"e": 0, "c": 32, "pu_h": 36, "pu_w": 40, "mv_int_x": 44, "mv_int_y": 46, "n_emi": 48,
                   "writes": 49, "status": 50, "reserved": 52}
    assert predictor.RES_NN_EXTERN == 0x08
    assert predictor.RES_NN_EXTERN & (RES_NN_STALE | RES_NN_UNINIT | RES_REJECTED | direct.RES_NN_DIRECT) == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_rows_are_what_the_net_read(name):
    g, rows, _ = golden_rows(name)
    engines, net, qp = _engines(g)
    want = g["results"]["nn_class"]
    wts = None if net is not None else weights.load_weights(qp)
    for i, r in enumerate(rows):
        e, c, h, w = r["e"], int(r["c"]), int(r["pu_h"]), int(r["pu_w"])
        got = engines[0].nn_net_forward(e, c, h, w)[0] if net is not None else engines[0].nn_class(wts, e, c, h, w)[0]
        assert got == want[i], (name, i, got, int(want[i]))
        if HAVE_REF:
            ref = engines[1].nn_net_class(e, c, h, w)[0] if net is not None else engines[1].nn_class(e, c, h, w)
            assert ref == want[i], (name, "reference", i, ref, int(want[i]))


@pytest.mark.parametrize("name", FIXTURES)
def test_state_out_is_the_oracles(name):
    g, rows, out = golden_rows(name)
    o = _engines(g)[0][0]
    for i, p in enumerate(g["pictures"]):
        o.set_picture(i, p)
    for i, lam in enumerate(g["lambdas"]):
        o.set_lambda(i, float(lam))
    if g["keys"].size:
        o.set_keys(g["keys"])
    o.nn_reset()
    n = len(g["jobs"])
    k = n // 3
    first = o.refine(g["jobs"][:k])
    mid = o.nn_get_state()
    rest = o.refine(g["jobs"][k:])
    assert np.array_equal(np.concatenate([first, rest])["nn_class"], g["results"]["nn_class"])
    assert np.array_equal(out, o.nn_get_state())
    # and chained: the rows of the second part from the state after the first are the rows of the whole
    reset = slot_reset_of(g)
    r1, s1 = predictor.rows_numpy(g["jobs"][:k], g["results"][:k], None, reset)
    assert np.array_equal(s1, mid)
    r2, s2 = predictor.rows_numpy(g["jobs"][k:], g["results"][k:], s1, reset)
    assert np.concatenate([r1, r2]).tobytes() == rows.tobytes() and np.array_equal(s2, out)


@pytest.mark.parametrize("name", FIXTURES)
def test_rows_carry_the_records_fields(name):
    g, rows, _ = golden_rows(name)
    jobs, res = g["jobs"], g["results"]
    emi = (jobs["flags"] & JOB_EMI) != 0
    assert (~emi).any(), "a job without FME_JOB_EMI"
    assert (emi & (res["n_emi"] < 8)).any(), "a job that pushes fewer than 8"
    own = np.where(emi[:, None] & (res["n_emi"][:, None] > np.arange(8)[None, :]), res["emi"], 0)
    if not slot_reset_of(g):
        assert (rows["e"] != own).any(axis=1).any(), "a job whose row differs from its own pushes"
    else:
        assert np.array_equal(rows["e"], own)
    for f in ("mv_int_x", "mv_int_y", "n_emi"):
        assert np.array_equal(rows[f], res[f]), f
    assert np.array_equal(rows["writes"] != 0, emi) and (rows["reserved"] == 0).all()
    # the ordinary run's stale / uninit bits are the rows' (the goldens store none: from the rule)
    stale = ~emi | (res["n_emi"] < 8)
    assert np.array_equal((rows["status"] & RES_NN_STALE) != 0, stale)
    assert (rows["status"] & ~np.uint16(RES_NN_STALE | RES_NN_UNINIT) == 0).all()
    # a job with all eight pushes reads its own record
    full = emi & (res["n_emi"] == 8)
    assert np.array_equal(rows["e"][full], res["emi"][full]) and np.array_equal(rows["c"][full], res["c"][full])
    assert np.array_equal(rows["pu_h"][emi], jobs["h"][emi]) and np.array_equal(rows["pu_w"][emi], jobs["w"][emi])
    # and back: the records fme_refine_at builds from the rows hold the golden's EMI fields
    back = predictor.records_of_rows(rows)
    for f in ("mv_int_x", "mv_int_y", "c", "emi", "n_emi"):
        assert np.array_equal(back[f], res[f]), f


@pytest.mark.parametrize("name", FIXTURES)
def test_refine_at_numpy_with_the_goldens_classes_is_direct_numpy(name):
    g, idx, surf = subset(name)
    jobs, res = g["jobs"][idx], g["results"][idx]
    want = direct.direct_numpy(jobs, res, surf, g["lambdas"])
    got = predictor.refine_at_numpy(jobs, res, res["nn_class"], surf, g["lambdas"])
    assert (got["status"] == direct.RES_NN_DIRECT | predictor.RES_NN_EXTERN).all()
    for f in RESULT_DTYPE.names:
        if f != "status":
            assert np.array_equal(got[f], want[f]), f
    # from the rows alone (no ordinary records) the same again
    _, rows, _ = golden_rows(name)
    again = predictor.refine_at_numpy(jobs, predictor.records_of_rows(rows[idx]), res["nn_class"], surf, g["lambdas"])
    assert again.tobytes() == got.tobytes()
    # another class moves the record with it; a class above 48 refuses the job alone
    cls = res["nn_class"].copy()
    cls[0], cls[1], cls[2] = (int(cls[0]) + 1) % 49, 49, 255
    other = predictor.refine_at_numpy(jobs, res, cls, surf, g["lambdas"])
    assert other[3:].tobytes() == got[3:].tobytes()
    assert other["nn_class"][0] == cls[0] and other["mv_x"][0] == 4 * int(res["mv_int_x"][0]) + int(cls[0]) % 7 - 3
    assert other["frac_cost"][0] == (surf["cost"] if surf.dtype.names else surf).reshape(len(idx), 49)[0, cls[0]]
    blank = np.zeros(1, RESULT_DTYPE)
    blank["status"] = RES_REJECTED
    assert other[1:3].tobytes() == np.repeat(blank, 2).tobytes()


def test_features_and_dataset_records():
    g, rows, _ = golden_rows(FIXTURES[0])
    x = predictor.features(rows)
    assert x.dtype == np.float32 and x.shape == (len(rows), 11)
    recs, _ = dataset.records(g["jobs"], g["results"])
    for k, n in enumerate(dataset.CONT_VARS):
        assert np.array_equal(x[:, k], recs[n].astype(np.float32)), n
    assert np.array_equal(x[:, 9], rows["pu_h"].astype(np.float32)) and np.array_equal(x[:, 10], rows["pu_w"].astype(np.float32))
    big = rows[:2].copy()
    big["e"][0, 3] = 0xFFFFFFFF
    assert predictor.features(big)[0, 3] == np.float32(4294967295.0)
    # records_from_rows is records() wherever the job has FME_JOB_EMI (the calls the reference logs)
    y = dataset.out_class(g["results"]["half_x"], g["results"]["half_y"], g["results"]["qtr_x"], g["results"]["qtr_y"])
    mine = dataset.records_from_rows(rows, y)
    emi = (g["jobs"]["flags"] & JOB_EMI) != 0
    assert mine[emi].tobytes() == recs[emi].tobytes()
    for n in dataset.CONT_VARS + ("y",):
        assert np.array_equal(mine[n], recs[n]), n
    with pytest.raises(ValueError):
        dataset.records_from_rows(rows, y[:-1])
