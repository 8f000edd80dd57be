"""The skip-mode RD check of the 2Nx2N merge candidates (include/fme_skip.h) over libfme_amd.so.

The numpy mirrors of fme_sse_task / fme_skip_params / fme_skip_req / fme_skip_res, the ctypes
prototypes of the header's entry points (bound on the handle runtime.load_library() returns; they
are additional exports, not part of runtime.ABI_SYMBOLS), wrappers that raise FmeError with the
library's code, and a plain numpy restatement of the distortion, weighting, cost and choice.
There is no CPU fallback: a library without these symbols raises FmeError.
"""
import ctypes as C

import numpy as np

from .merge import MERGE_CAND_DTYPE, MRG_MAX_CAND
from .runtime import FmeError, _check, _ptr

SKIP_NONE = 0xFF
NO_SSE = 0xFFFFFFFF

SSE_TASK_DTYPE = np.dtype([
    ("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("org_id", "u1"), ("flags", "u1"),
    ("cu_x", "<u2"), ("cu_y", "<u2"), ("ref_id", "u1", (2,)), ("reserved", "<u2"), ("mv", "<i2", (2, 2)),
])
assert SSE_TASK_DTYPE.itemsize == 24

SKIP_PARAMS_DTYPE = np.dtype([("lambda", "<f8"), ("chroma_weight", "<f8", (2,))])
assert SKIP_PARAMS_DTYPE.itemsize == 24

SKIP_REQ_DTYPE = np.dtype([
    ("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("org_id", "u1"), ("n_cand", "u1"),
    ("cand_mask", "u1"), ("flags", "u1"), ("reserved", "<u2"),
    ("cand", MERGE_CAND_DTYPE, (MRG_MAX_CAND,)), ("bits", "<u4", (MRG_MAX_CAND,)), ("reserved2", "<u4"),
])
assert SKIP_REQ_DTYPE.itemsize == 96

SKIP_RES_DTYPE = np.dtype([
    ("best_cost", "<f8"), ("cand_cost", "<f8", (MRG_MAX_CAND,)), ("cand_sse", "<u4", (MRG_MAX_CAND, 3)),
    ("cand_dist", "<u4", (MRG_MAX_CAND,)), ("best", "u1"), ("reserved", "u1", (7,)),
])
assert SKIP_RES_DTYPE.itemsize == 136

# The functions include/fme_skip.h declares (tests/test_skip_abi.py checks the header against this).
SKIP_SYMBOLS = ("fme_pred_sse", "fme_pred_sse_device", "fme_pred_sse_invalid_count", "fme_pred_sse_last_ms",
                "fme_skip_estimate")


def bind(lib):
    """Set the prototypes of the fme_skip.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_skip_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_pred_sse": (I, [P, P, P, I, P]),
        "fme_pred_sse_device": (I, [P, P, P, I, P]),
        "fme_pred_sse_invalid_count": (I, [P]),
        "fme_pred_sse_last_ms": (I, [P, P]),
        "fme_skip_estimate": (I, [P, P, P, P, I, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_skip.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_skip_bound = True
    return lib


def pred_sse(ctx, tasks, stream=None, out=None):
    """fme_pred_sse: uint32 [n, 3] (Y, Cb, Cr, unweighted) of the SSE_TASK_DTYPE tasks, host arrays.
    out: an array to receive them (a rejected batch leaves it untouched)."""
    lib = bind(ctx.lib)
    tasks = np.ascontiguousarray(tasks, dtype=SSE_TASK_DTYPE)
    sse = np.zeros((len(tasks), 3), np.uint32) if out is None else out
    assert sse.dtype == np.uint32 and sse.flags.c_contiguous and sse.shape == (len(tasks), 3)
    _check(lib, lib.fme_pred_sse(ctx.h, _ptr(tasks), _ptr(sse), len(tasks), stream))
    return sse


def pred_sse_device(ctx, d_tasks, d_sse, n=None, stream=None):
    """fme_pred_sse_device on torch tensors: d_tasks a uint8 device tensor holding n SSE_TASK_DTYPE
    records, d_sse a 4-byte-element device tensor of at least 3 n elements (written in stream order;
    an invalid task's three slots are 0xFFFFFFFF).  No host synchronisation."""
    lib = bind(ctx.lib)
    if n is None:
        n = d_tasks.numel() * d_tasks.element_size() // SSE_TASK_DTYPE.itemsize
    if d_tasks.numel() * d_tasks.element_size() < n * SSE_TASK_DTYPE.itemsize or \
            d_sse.numel() * d_sse.element_size() < 12 * n:
        raise FmeError(-1, "pred_sse_device: tensors shorter than n tasks")
    _check(lib, lib.fme_pred_sse_device(ctx.h, C.c_void_p(d_tasks.data_ptr()), C.c_void_p(d_sse.data_ptr()), int(n),
                                        stream))


def pred_sse_invalid_count(ctx):
    lib = bind(ctx.lib)
    rc = lib.fme_pred_sse_invalid_count(ctx.h)
    if rc < 0:
        _check(lib, rc)
    return rc


def pred_sse_last_ms(ctx):
    lib = bind(ctx.lib)
    ms = C.c_float()
    _check(lib, lib.fme_pred_sse_last_ms(ctx.h, C.byref(ms)))
    return ms.value


def make_params(lam, chroma_weight):
    p = np.zeros((), SKIP_PARAMS_DTYPE)
    p["lambda"] = lam
    p["chroma_weight"] = chroma_weight
    return p


def skip_estimate(ctx, params, reqs, stream=None):
    """fme_skip_estimate: one SKIP_RES_DTYPE record per SKIP_REQ_DTYPE request; params a
    SKIP_PARAMS_DTYPE record (make_params)."""
    lib = bind(ctx.lib)
    params = np.ascontiguousarray(params, dtype=SKIP_PARAMS_DTYPE).reshape(1)
    reqs = np.ascontiguousarray(reqs, dtype=SKIP_REQ_DTYPE)
    res = np.zeros(len(reqs), SKIP_RES_DTYPE)
    _check(lib, lib.fme_skip_estimate(ctx.h, _ptr(params), _ptr(reqs), _ptr(res), len(reqs), stream))
    return res


# ---- plain restatements (the fixtures' generator and the CPU tests) --------------------------------

def sse_numpy(org, pred, bit_depth=8):
    """TComRdCost::getDistPart with DF_SSE on one block, before the chroma weight
    (TComRdCost.cpp:327-345): xGetSSE / xGetSSE4..64 (861-1205) all sum, over every sample,
    (org - cur)^2 >> uiShift with uiShift = DISTORTION_PRECISION_ADJUSTMENT((bitDepth - 8) << 1)
    (:875, each sample's square shifted, :884), in Distortion = UInt (TypeDef.h:239)."""
    d = np.asarray(org, np.int64) - np.asarray(pred, np.int64)
    return int(((d * d) >> ((bit_depth - 8) << 1)).sum()) & 0xFFFFFFFF


def eval_mask(req):
    return int(req["cand_mask"]) & ((1 << int(req["n_cand"])) - 1)


def weighted_numpy(weight, sse):
    """(Distortion)(m_distortionWeight[compID] * sse) (TComRdCost.cpp:343): a double product,
    truncated toward zero."""
    return int(float(weight) * float(int(sse)))


def skip_decide_numpy(req, sse, params):
    """Steps 3-5 for one request; sse: [m, 3] of its evaluated candidates in index order.
    distortion = Y + Cb' + Cr' in UInt (TEncSearch.cpp:5294-5303); calcRdCost with DF_DEFAULT in
    COST_STANDARD_LOSSY = distortion + bits * lambda in doubles (TComRdCost.cpp:99);
    xCheckBestMode takes a candidate only when strictly below the best so far (TEncCu.cpp:1239)."""
    r = np.zeros((), SKIP_RES_DTYPE)
    r["best"], r["best_cost"] = SKIP_NONE, np.inf
    r["cand_cost"] = np.inf
    r["cand_sse"] = r["cand_dist"] = NO_SSE
    lam = float(params["lambda"])
    w = [float(params["chroma_weight"][0]), float(params["chroma_weight"][1])]
    m, at = eval_mask(req), 0
    for k in range(MRG_MAX_CAND):
        if not (m >> k) & 1:
            continue
        s = [int(v) for v in sse[at]]
        dist = (s[0] + weighted_numpy(w[0], s[1]) + weighted_numpy(w[1], s[2])) & 0xFFFFFFFF
        cost = float(dist) + float(int(req["bits"][k])) * lam
        r["cand_sse"][k], r["cand_dist"][k], r["cand_cost"][k] = s, dist, cost
        if cost < float(r["best_cost"]):
            r["best"], r["best_cost"] = k, cost
        at += 1
    return r


def expand_requests(reqs):
    """The requests' SSE_TASK_DTYPE tasks in fme_skip_estimate's order (the evaluated candidates in
    index order; the CU is its own clipMv origin), and each request's first task."""
    tasks, first = [], []
    for q in reqs:
        first.append(len(tasks))
        m = eval_mask(q)
        for k in range(int(q["n_cand"])):
            if not (m >> k) & 1:
                continue
            c = q["cand"][k]
            d = int(c["inter_dir"])
            t = np.zeros((), SSE_TASK_DTYPE)
            for f in ("x", "y", "w", "h", "org_id"):
                t[f] = q[f]
            t["cu_x"], t["cu_y"] = q["x"], q["y"]
            t["flags"] = d & 3
            for l in range(2):
                if d & (1 << l):
                    t["ref_id"][l] = c["ref_id"][l]
                    t["mv"][l] = c["mv"][l]
            tasks.append(t)
    return np.array(tasks, dtype=SSE_TASK_DTYPE).reshape(-1), np.array(first, np.int64)


def block_sse(org_planes, pred_planes, task, bit_depth=8):
    """[Y, Cb, Cr] SSE of one task's block: org_planes / pred_planes are (Y, Cb, Cr) pictures, the
    4:2:0 chroma block at (x >> 1, y >> 1) of size (w >> 1, h >> 1)."""
    x, y, w, h = (int(task[f]) for f in ("x", "y", "w", "h"))
    out = []
    for c in range(3):
        s = 0 if c == 0 else 1
        sl = (slice(y >> s, (y >> s) + (h >> s)), slice(x >> s, (x >> s) + (w >> s)))
        out.append(sse_numpy(org_planes[c][sl], pred_planes[c][sl], bit_depth))
    return out
