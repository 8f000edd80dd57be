"""The sub-pel cost surface (include/fme_surface.h) over libfme_amd.so: the distortion and cost of all
49 quarter-pel positions within +-3/4 pel of a job's integer MV.

The numpy mirrors of fme_surface / fme_surface_pick, the ctypes prototypes of the header's entry
points (bound on the handle runtime.load_library() returns; they are additional exports, not part
of runtime.ABI_SYMBOLS), wrappers that raise FmeError with the library's code, the host arithmetic
of csrc/fme_surface_host.h restated on arrays (the replay of xPatternRefinement's two stages, the
regret record) and a plain numpy restatement of one job's surface.  There is no CPU fallback: a
library without these symbols raises FmeError.
"""
import ctypes as C
import math

import numpy as np

from .abi import JOB_DTYPE, JOB_LOSSLESS
from .merge import _LUMA_TAPS, dist_numpy
from .runtime import FmeError, _check, _ptr

POINTS = 49
NO_PROBE = 0xFF
NO_COST = 0xFFFFFFFF

SURFACE_DTYPE = np.dtype([("dist", "<u4", (POINTS,)), ("cost", "<u4", (POINTS,))])
assert SURFACE_DTYPE.itemsize == 392

PICK_DTYPE = np.dtype([("min_cost", "<u4"), ("probe_cost", "<u4", (2,)), ("min_idx", "u1"), ("probe", "u1", (2,)),
                       ("status", "u1")])
assert PICK_DTYPE.itemsize == 16

REPLAY_DTYPE = np.dtype([("half_x", "i1"), ("half_y", "i1"), ("qtr_x", "i1"), ("qtr_y", "i1"),
                         ("half_cost", "<u4"), ("frac_cost", "<u4")])
REGRET_DTYPE = np.dtype([("search_cost", "<u4"), ("class_cost", "<u4"), ("min_cost", "<u4"),
                         ("search_idx", "u1"), ("min_idx", "u1")])

# The functions include/fme_surface.h declares.
SURFACE_SYMBOLS = ("fme_cost_surface", "fme_cost_surface_device", "fme_cost_surface_invalid_count",
                   "fme_cost_surface_last_ms")

# xPatternRefinement's visiting orders (TEncSearch.cpp:212-236): s_acMvRefineH, s_acMvRefineQ
REFINE_H = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))
REFINE_Q = ((0, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1))


def index(dx, dy):
    """FME_SURF_INDEX: the position index of quarter-pel offset (dx, dy) = its NN_pred class."""
    return (np.asarray(dy) + 3) * 7 + np.asarray(dx) + 3


def offset(idx):
    """(dx, dy) of a position index."""
    idx = np.asarray(idx)
    return idx % 7 - 3, idx // 7 - 3


def bind(lib):
    """Set the prototypes of the fme_surface.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_surface_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_cost_surface": (I, [P, P, P, P, P, I, P]),
        "fme_cost_surface_device": (I, [P, P, P, P, P, I, P]),
        "fme_cost_surface_invalid_count": (I, [P]),
        "fme_cost_surface_last_ms": (I, [P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_surface.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_surface_bound = True
    return lib


def cost_surface(ctx, jobs, probes=None, surface=True, pick=True, stream=None, out=None):
    """fme_cost_surface on host arrays: (SURFACE_DTYPE[n] or None, PICK_DTYPE[n] or None).
    probes: uint8 [n, 2] position indices (NO_PROBE: none) or None.  out: a (surface, pick) pair of
    arrays to receive the records (a rejected batch leaves them untouched)."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    n = len(jobs)
    if probes is not None:
        probes = np.ascontiguousarray(probes, dtype=np.uint8)
        assert probes.shape == (n, 2)
    if out is not None:
        surf, pk = out
    else:
        surf = np.zeros(n, SURFACE_DTYPE) if surface else None
        pk = np.zeros(n, PICK_DTYPE) if pick else None
    for a, dt in ((surf, SURFACE_DTYPE), (pk, PICK_DTYPE)):
        assert a is None or (a.dtype == dt and a.flags.c_contiguous and a.shape == (n,))
    _check(lib, lib.fme_cost_surface(ctx.h, _ptr(jobs), None if probes is None else _ptr(probes),
                                     None if surf is None else _ptr(surf), None if pk is None else _ptr(pk), n, stream))
    return surf, pk


def _dev(t, nbytes, what):
    if t is None:
        return None
    if t.numel() * t.element_size() < nbytes:
        raise FmeError(-1, f"cost_surface_device: {what} tensor shorter than n records")
    return C.c_void_p(t.data_ptr())


def cost_surface_device(ctx, d_jobs, d_probe, d_surf, d_pick, n=None, stream=None):
    """fme_cost_surface_device on torch tensors: d_jobs a uint8 device tensor holding n JOB_DTYPE
    records, d_probe None or 2 n bytes, d_surf None or 392 n bytes, d_pick None or 16 n bytes
    (written in stream order; an invalid job's words are 0xFFFFFFFF and its status 1).  No host
    synchronisation."""
    lib = bind(ctx.lib)
    if n is None:
        n = d_jobs.numel() * d_jobs.element_size() // JOB_DTYPE.itemsize
    n = int(n)
    _check(lib, lib.fme_cost_surface_device(ctx.h, _dev(d_jobs, n * JOB_DTYPE.itemsize, "job"), _dev(d_probe, 2 * n, "probe"),
                                            _dev(d_surf, n * SURFACE_DTYPE.itemsize, "surface"),
                                            _dev(d_pick, n * PICK_DTYPE.itemsize, "pick"), n, stream))


def cost_surface_invalid_count(ctx):
    lib = bind(ctx.lib)
    rc = lib.fme_cost_surface_invalid_count(ctx.h)
    if rc < 0:
        _check(lib, rc)
    return rc


def cost_surface_last_ms(ctx):
    lib = bind(ctx.lib)
    ms = C.c_float()
    _check(lib, lib.fme_cost_surface_last_ms(ctx.h, C.byref(ms)))
    return ms.value


def jobs_at_results(jobs, results):
    """The jobs whose surfaces are the ones a refinement saw: mv := fme_result.mv_int (the integer
    MV after the EMI step)."""
    j = np.array(jobs, dtype=JOB_DTYPE, copy=True)
    j["mv_x"] = results["mv_int_x"]
    j["mv_y"] = results["mv_int_y"]
    return j


# ---- the host arithmetic of csrc/fme_surface_host.h on arrays ----------------------------------------

def _cost_rows(surface):
    a = np.asarray(surface)
    c = a["cost"] if a.dtype.names else a
    return np.ascontiguousarray(c, dtype=np.uint32).reshape(-1, POINTS)


def _stage(cost, bx, by, step, order):
    """One xPatternRefinement stage on every row: the nine offsets of `order` times `step` around
    (bx, by), first strict minimum."""
    n = len(cost)
    rows = np.arange(n)
    cand = np.stack([cost[rows, index(bx + step * ox, by + step * oy)] for ox, oy in order], axis=1)
    k = np.argmin(cand, axis=1)   # the first of equal minima: strict < in visiting order
    o = np.array(order, np.int64)
    return o[k, 0], o[k, 1], cand[rows, k]


def replay_search(surface):
    """What xPatternSearchFracDIF decides on each surface (REPLAY_DTYPE[n]): the half stage over
    s_acMvRefineH at step 2, then the quarter stage over s_acMvRefineQ around the half pick."""
    cost = _cost_rows(surface)
    r = np.zeros(len(cost), REPLAY_DTYPE)
    zero = np.zeros(len(cost), np.int64)
    hx, hy, hc = _stage(cost, zero, zero, 2, REFINE_H)
    qx, qy, qc = _stage(cost, 2 * hx, 2 * hy, 1, REFINE_Q)
    r["half_x"], r["half_y"], r["half_cost"] = hx, hy, hc
    r["qtr_x"], r["qtr_y"], r["frac_cost"] = qx, qy, qc
    return r


def pick_numpy(surface, probes=None):
    """The pick and probe rule on arrays (PICK_DTYPE[n])."""
    cost = _cost_rows(surface)
    n = len(cost)
    p = np.zeros(n, PICK_DTYPE)
    p["min_idx"] = np.argmin(cost, axis=1)
    p["min_cost"] = cost[np.arange(n), p["min_idx"]]
    pr = np.full((n, 2), NO_PROBE, np.uint8) if probes is None else np.asarray(probes, np.uint8)
    p["probe"] = pr
    for k in range(2):
        have = pr[:, k] < POINTS
        p["probe_cost"][:, k] = np.where(have, cost[np.arange(n), np.where(have, pr[:, k], 0)], NO_COST)
    return p


def regret(results, surface):
    """The regret record of every job (REGRET_DTYPE[n]): the cost at the search's pick
    (2 half + qtr; equals frac_cost when the surface is centred on mv_int), at the job's nn_class
    (NO_COST for class 255) and the minimum with its index."""
    cost = _cost_rows(surface)
    n = len(cost)
    g = np.zeros(n, REGRET_DTYPE)
    rows = np.arange(n)
    g["search_idx"] = index(2 * results["half_x"].astype(np.int64) + results["qtr_x"],
                            2 * results["half_y"].astype(np.int64) + results["qtr_y"])
    g["search_cost"] = cost[rows, g["search_idx"]]
    cls = np.asarray(results["nn_class"]).astype(np.int64)
    have = cls < POINTS
    g["class_cost"] = np.where(have, cost[rows, np.where(have, cls, 0)], NO_COST)
    g["min_idx"] = np.argmin(cost, axis=1)
    g["min_cost"] = cost[rows, g["min_idx"]]
    return g


# ---- plain restatement (the fixtures' generator and the CPU tests) -----------------------------------

def _eg_bits(v):
    """TComRdCost::xGetComponentBits (TComRdCost.cpp:172-185)."""
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 2 * t.bit_length() - 1


def mv_cost_numpy(motion_lambda, bits):
    """TComRdCost::getCost (TComRdCost.h:165): (UInt)(mlambda * bits / 65536.0)."""
    return int((float(motion_lambda) * float(bits)) / 65536.0)


def surface_numpy(pictures, keys, lambdas, job, use_hadamard, bit_depth=8):
    """One job's surface restated (a SURFACE_DTYPE scalar): the two-stage luma filter of
    merge.predict_numpy at the 49 quarter-pel MVs (4 mv + (dx, dy)) with no clipMv and replicated
    edges, merge.dist_numpy against the original or the key block, and the MV cost in UInt
    arithmetic.  pictures: {slot: [H, W] samples} (or an array of planes); keys: the int16 key
    buffer; lambdas: what fme_set_lambda was given per id (the motion lambda is 65536 sqrt(lambda))."""
    x, y, w, h = (int(job[f]) for f in ("x", "y", "w", "h"))
    mvx, mvy, px, py = (int(job[f]) for f in ("mv_x", "mv_y", "mvp_x", "mvp_y"))
    pic = np.asarray(pictures[int(job["ref_id"])])
    ph, pw = pic.shape
    half, maxv, sh = 1 << (bit_depth - 1), (1 << bit_depth) - 1, 20 - bit_depth
    rows = np.clip(np.arange(y + mvy - 4, y + mvy + h + 8), 0, ph - 1)
    cols = np.clip(np.arange(x + mvx - 4, x + mvx + w + 8), 0, pw - 1)
    win = pic[np.ix_(rows, cols)].astype(np.int64) - half
    ko = int(job["key_offset"])
    if ko >= 0:
        target = np.asarray(keys[ko:ko + w * h], np.int64).reshape(h, w)
    else:
        target = np.asarray(pictures[int(job["org_id"])])[y:y + h, x:x + w].astype(np.int64)
    had = bool(use_hadamard) and not int(job["flags"]) & JOB_LOSSLESS
    ml = 65536.0 * math.sqrt(float(lambdas[int(job["lambda_id"])]))
    s = np.zeros((), SURFACE_DTYPE)
    for dx in range(-3, 4):
        ox, ch = 1 + (dx >> 2), _LUMA_TAPS[dx & 3]   # window column of the first tap of output column 0
        s1 = sum(int(ch[k]) * win[:, ox + k:ox + k + w] for k in range(8)) >> (bit_depth - 8)
        for dy in range(-3, 4):
            oy, cv = 1 + (dy >> 2), _LUMA_TAPS[dy & 3]
            s2 = sum(int(cv[k]) * s1[oy + k:oy + k + h, :] for k in range(8))
            pred = np.clip(((s2 + (1 << (sh - 1))) >> sh) + half, 0, maxv)
            i = int(index(dx, dy))
            d = dist_numpy(target, pred, had, bit_depth)
            bits = _eg_bits(4 * mvx + dx - px) + _eg_bits(4 * mvy + dy - py)
            s["dist"][i] = d
            s["cost"][i] = (d + mv_cost_numpy(ml, bits)) & 0xFFFFFFFF
    return s


def surfaces_numpy(pictures, keys, lambdas, jobs, use_hadamard, bit_depth=8):
    """surface_numpy of every job (SURFACE_DTYPE[n])."""
    out = np.zeros(len(jobs), SURFACE_DTYPE)
    for i, j in enumerate(jobs):
        out[i] = surface_numpy(pictures, keys, lambdas, j, use_hadamard, bit_depth)
    return out
