"""Candidate-set refinement (include/fme_among.h) over libfme_amd.so: per job the best of up to 8
sub-pel positions, the two-layer net's K highest outputs as such a list, and the two chained.

The ctypes prototypes of the header's entry points (additional exports, bound on the handle
runtime.load_library() returns) with wrappers that raise FmeError; and what those entry points must
produce restated in numpy: among_numpy on predictor.refine_at_numpy slot by slot, rank_numpy as the
float32 sequential-k forward of NN_pred() over rows, topk_numpy as their composition on
predictor.rows_numpy.  There is no CPU fallback: a library without these symbols raises FmeError.
"""
import ctypes as C

import numpy as np

from . import direct, predictor, weights
from .abi import JOB_DTYPE, RES_NN_STALE, RES_NN_UNINIT, RES_REJECTED, RESULT_DTYPE
from .predictor import NN_ROW_DTYPE
from .runtime import FmeError, _check, _ptr
from .surface import POINTS

AMONG_MAX = 8
AMONG_EMPTY = 0xFF
RES_NN_AMONG = 0x10
NONE = 0xFFFFFFFF          # the cost word of an empty slot / a refused job
AMONG_STATUS = direct.RES_NN_DIRECT | predictor.RES_NN_EXTERN | RES_NN_AMONG
TOPK_STATUS = direct.RES_NN_DIRECT | RES_NN_AMONG
LAST_MS_NAMES = ("emi", "rows", "rank", "evaluation", "batch")

# The functions include/fme_among.h declares.
AMONG_SYMBOLS = ("fme_refine_among", "fme_refine_among_device", "fme_refine_among_mv_device",
                 "fme_refine_among_status", "fme_nn_rank_device", "fme_refine_topk", "fme_refine_topk_device",
                 "fme_refine_topk_mv_device", "fme_among_last_ms")


def bind(lib):
    """Set the prototypes of the fme_among.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_among_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_refine_among": (I, [P, P, P, P, I, P, P, I, P]),
        "fme_refine_among_device": (I, [P, P, P, P, I, P, P, I, P]),
        "fme_refine_among_mv_device": (I, [P, P, P, P, I, P, P, I, P]),
        "fme_refine_among_status": (I, [P]),
        "fme_nn_rank_device": (I, [P, P, P, I, I, P]),
        "fme_refine_topk": (I, [P, P, P, I, P, P, I, P]),
        "fme_refine_topk_device": (I, [P, P, P, I, P, P, I, P]),
        "fme_refine_topk_mv_device": (I, [P, P, P, I, P, P, I, P]),
        "fme_among_last_ms": (I, [P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_among.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_among_bound = True
    return lib


_dev = direct._dev


def _lists(cand, n):
    """The candidate lists as a contiguous uint8 [n, k]."""
    c = np.ascontiguousarray(cand, dtype=np.uint8)
    if c.ndim != 2 or len(c) != n:
        raise ValueError("one list of k slots per job: cand is [n, k]")
    return c


def refine_among(ctx, jobs, cand, rows=None, stream=None, out=None, costs=True):
    """fme_refine_among on host arrays: (RESULT_DTYPE[n] (written into `out` when given), the slots'
    costs uint32 [n, k], or None with costs=False)."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    c = _lists(cand, len(jobs))
    if rows is not None and len(rows) != len(jobs):
        raise ValueError("refine_among: one row per job")
    r = None if rows is None else np.ascontiguousarray(rows, dtype=NN_ROW_DTYPE)
    res = np.zeros(len(jobs), dtype=RESULT_DTYPE) if out is None else out
    cc = np.zeros(c.shape, np.uint32) if costs else None
    _check(lib, lib.fme_refine_among(ctx.h, _ptr(jobs), None if r is None else _ptr(r), _ptr(c), c.shape[1], _ptr(res),
                                     None if cc is None else _ptr(cc), len(jobs), stream))
    return res, cc


def refine_among_device(ctx, d_jobs, d_rows, d_cand, k, d_res, d_cand_cost, n, stream=None):
    """fme_refine_among_device: d_rows may be None (the EMI step runs), d_cand_cost may be None."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_among_device(ctx.h, _dev(d_jobs), _dev(d_rows), _dev(d_cand), int(k), _dev(d_res),
                                            _dev(d_cand_cost), int(n), stream))


def refine_among_mv_device(ctx, d_jobs, d_rows, d_cand, k, d_out, d_cand_cost, n, stream=None):
    """fme_refine_among_mv_device: the same with the 16-byte MV_RESULT_DTYPE records."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_among_mv_device(ctx.h, _dev(d_jobs), _dev(d_rows), _dev(d_cand), int(k), _dev(d_out),
                                               _dev(d_cand_cost), int(n), stream))


def refine_among_status(ctx):
    """Jobs the last among / top-K batch refused one by one (waits for it)."""
    lib = bind(ctx.lib)
    rc = lib.fme_refine_among_status(ctx.h)
    if rc < 0:
        _check(lib, rc)
    return rc


def nn_rank_device(ctx, d_rows, d_cand, k, n, stream=None):
    """fme_nn_rank_device: n rows in, n*k candidate bytes out."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_nn_rank_device(ctx.h, _dev(d_rows), _dev(d_cand), int(k), int(n), stream))


def refine_topk(ctx, jobs, k, stream=None):
    """fme_refine_topk on host arrays: (RESULT_DTYPE[n], the candidates uint8 [n, k], their costs
    uint32 [n, k])."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    n = len(jobs)
    res = np.zeros(n, dtype=RESULT_DTYPE)
    cand = np.zeros((n, max(int(k), 0)), np.uint8)
    cc = np.zeros(cand.shape, np.uint32)
    _check(lib, lib.fme_refine_topk(ctx.h, _ptr(jobs), _ptr(res), int(k), _ptr(cand), _ptr(cc), n, stream))
    return res, cand, cc


def refine_topk_device(ctx, d_jobs, d_res, k, d_cand, d_cand_cost, n, stream=None):
    """fme_refine_topk_device: d_cand and d_cand_cost may be None."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_topk_device(ctx.h, _dev(d_jobs), _dev(d_res), int(k), _dev(d_cand), _dev(d_cand_cost),
                                           int(n), stream))


def refine_topk_mv_device(ctx, d_jobs, d_out, k, d_cand, d_cand_cost, n, stream=None):
    """fme_refine_topk_mv_device: the same with the 16-byte MV_RESULT_DTYPE records."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_topk_mv_device(ctx.h, _dev(d_jobs), _dev(d_out), int(k), _dev(d_cand),
                                              _dev(d_cand_cost), int(n), stream))


def last_ms(ctx):
    """{phase: device ms} of the last among / rank / top-K call with profiling on (LAST_MS_NAMES)."""
    lib = bind(ctx.lib)
    ms = np.zeros(5, np.float32)
    _check(lib, lib.fme_among_last_ms(ctx.h, _ptr(ms)))
    return dict(zip(LAST_MS_NAMES, ms.tolist()))


# ---- the records and the ranking restated in numpy -----------------------------------------------------

def refused_lists(cand):
    """bool [n]: lists fme_refine_among refuses (a slot in 49..254, or no class at all)."""
    c = np.asarray(cand).astype(np.int64)
    empty = c == AMONG_EMPTY
    return ((c >= POINTS) & ~empty).any(axis=1) | empty.all(axis=1)


def pick_numpy(cand, cand_cost):
    """int [n]: the chosen slot of every list, the first of least cost among its non-empty slots
    (0 where every slot is empty)."""
    empty = np.asarray(cand).astype(np.int64) == AMONG_EMPTY
    masked = np.where(empty, np.int64(1) << 40, np.asarray(cand_cost).astype(np.int64))
    return np.argmin(masked, axis=1)      # the first index of the minimum


def among_numpy(jobs, results, cand, surfaces, lambdas):
    """(records RESULT_DTYPE[n], cand_cost uint32 [n, k]) fme_refine_among must give: slot by slot
    predictor.refine_at_numpy of the slot's classes (results: an ordinary refinement's records, or
    predictor.records_of_rows), the first slot of least frac_cost chosen; a refused list's record is 0
    but for RES_REJECTED and its costs all ones, as an empty slot's."""
    c = _lists(cand, len(jobs)).astype(np.int64)
    n, k = c.shape
    if not 1 <= k <= AMONG_MAX:
        raise ValueError("among_numpy: k is 1..8")
    empty = c == AMONG_EMPTY
    refused = refused_lists(c)
    off = empty | refused[:, None]
    slots = [predictor.refine_at_numpy(jobs, results, np.where(off[:, s], 24, c[:, s]), surfaces, lambdas)
             for s in range(k)]
    cost = np.stack([r["frac_cost"] for r in slots], axis=1).astype(np.uint32)
    cost[off] = NONE
    chosen = pick_numpy(np.where(off, AMONG_EMPTY, c), cost)
    out = np.zeros(n, RESULT_DTYPE)
    for s in range(k):
        out[chosen == s] = slots[s][chosen == s]
    out["status"] = AMONG_STATUS
    if refused.any():
        blank = np.zeros(1, RESULT_DTYPE)
        blank["status"] = RES_REJECTED
        out[refused] = blank[0]
    return out, cost


_ROW_H = {4: 1, 8: 2, 16: 3, 12: 4, 24: 5, 32: 6, 64: 7}
_ROW_W = {4: 1, 8: 2, 12: 3, 16: 4, 24: 5, 32: 6, 64: 7}


def logits_numpy(params, rows):
    """float32 [n, 49]: NN_pred()'s outputs for rows of NN inputs.  float32, every dot product summed
    in k order, a separate rounding per multiply and per add (each numpy float32 operation rounds
    once), ReLU then x * gamma + beta: the arithmetic of the NN tail."""
    rows = np.asarray(rows)
    n = len(rows)
    t = weights.unpack(params)
    f32 = np.float32
    rh = np.array([_ROW_H.get(int(v), 0) for v in rows["pu_h"]], np.int64)
    rw = np.array([_ROW_W.get(int(v), 0) for v in rows["pu_w"]], np.int64)
    x = [t["embs0"][rh, j].astype(f32) for j in range(4)] + [t["embs1"][rw, j].astype(f32) for j in range(4)]
    e = rows["e"]
    raw = [e[:, 0], e[:, 1], e[:, 2], e[:, 3], rows["c"], e[:, 4], e[:, 5], e[:, 6], e[:, 7]]
    for j in range(9):
        v = raw[j].astype(f32)
        v = (v - f32(t["mean"][j])) / f32(t["stdev"][j])
        x.append(v * f32(t["BN_gamma_in"][j]))

    def layer(x, w, b, g=None, be=None):
        out = []
        for r in range(w.shape[0]):
            s = np.zeros(n, f32)
            for j in range(w.shape[1]):
                s = s + f32(w[r, j]) * x[j]
            s = s + f32(b[r])
            if g is not None:
                s = np.where(s < 0, f32(0), s)
                s = s * f32(g[r]) + f32(be[r])
            out.append(s)
        return out

    x1 = layer(x, t["in_h1"], t["b1"], t["BN_gamma_1"], t["BN_beta_1"])
    x2 = layer(x1, t["h1_h2"], t["b2"], t["BN_gamma_2"], t["BN_beta_2"])
    out = np.stack(layer(x2, t["h2_out"], t["bout"]), axis=1) if n else np.zeros((0, POINTS), f32)
    assert out.dtype == f32
    return out


def order_numpy(logits, k):
    """uint8 [n, k]: the k classes of highest output, the highest first, equal outputs the lower class
    first (a stable descending sort)."""
    return np.argsort(-np.asarray(logits), axis=1, kind="stable")[:, :k].astype(np.uint8)


def rank_numpy(params, rows, k):
    """uint8 [n, k]: what fme_nn_rank_device must give for `rows`; a row marked RES_REJECTED gets
    AMONG_EMPTY in every slot."""
    if not 1 <= k <= AMONG_MAX:
        raise ValueError("rank_numpy: k is 1..8")
    rows = np.asarray(rows)
    out = order_numpy(logits_numpy(params, rows), k)
    out[(rows["status"] & RES_REJECTED) != 0] = AMONG_EMPTY
    return out


def topk_numpy(jobs, results, params, k, surfaces, lambdas, state_in=None):
    """(records, cand uint8 [n, k], cand_cost uint32 [n, k], state_out uint32[12]) fme_refine_topk must
    give: predictor.rows_numpy of an ordinary refinement's records and the NN state carried in,
    rank_numpy of those rows, among_numpy of the rows' records; status is the row's STALE / UNINIT bits
    plus RES_NN_DIRECT | RES_NN_AMONG."""
    rows, state = predictor.rows_numpy(jobs, results, state_in)
    cand = rank_numpy(params, rows, k)
    out, cost = among_numpy(jobs, predictor.records_of_rows(rows), cand, surfaces, lambdas)
    out["status"] = (rows["status"] & (RES_NN_STALE | RES_NN_UNINIT)) | TOPK_STATUS
    return out, cand, cost, state
