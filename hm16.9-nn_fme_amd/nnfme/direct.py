"""NN-direct refinement (include/fme_direct.h) over libfme_amd.so: per job the EMI step, NN_pred()
and one sub-pel evaluation at the net's own position, instead of xPatternSearchFracDIF's 17.

The ctypes prototypes of the header's entry points (bound on the handle runtime.load_library()
returns; they are additional exports, not part of runtime.ABI_SYMBOLS), wrappers that raise FmeError
with the library's code, the class -> half / quarter split of csrc/fme_direct_host.h on arrays, and
direct_numpy: the records a direct batch must produce, built from an ordinary refinement's records,
the cost surfaces centred on its integer MVs and a plain restatement of xMotionEstimation's tail.
There is no CPU fallback: a library without these symbols raises FmeError.
"""
import ctypes as C
import math

import numpy as np

from .abi import JOB_BIPRED, JOB_DTYPE, MV_RESULT_DTYPE, RESULT_DTYPE
from .runtime import FmeError, _check, _ptr
from .surface import POINTS, _cost_rows, _eg_bits, mv_cost_numpy

RES_NN_DIRECT = 0x04
LAST_MS_NAMES = ("emi", "class", "evaluation", "batch")

# The functions include/fme_direct.h declares.
DIRECT_SYMBOLS = ("fme_refine_direct", "fme_refine_direct_device", "fme_refine_direct_mv_device",
                  "fme_refine_direct_last_ms")


def bind(lib):
    """Set the prototypes of the fme_direct.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_direct_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_refine_direct": (I, [P, P, P, I, P]),
        "fme_refine_direct_device": (I, [P, P, P, I, P]),
        "fme_refine_direct_mv_device": (I, [P, P, P, I, P]),
        "fme_refine_direct_last_ms": (I, [P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_direct.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_direct_bound = True
    return lib


def refine_direct(ctx, jobs, stream=None):
    """fme_refine_direct on host arrays: RESULT_DTYPE[n]."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    res = np.zeros(len(jobs), dtype=RESULT_DTYPE)
    _check(lib, lib.fme_refine_direct(ctx.h, _ptr(jobs), _ptr(res), len(jobs), stream))
    return res


def _dev(t):
    """A device address: an integer, or anything with data_ptr() (a torch tensor)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def refine_direct_device(ctx, d_jobs, d_res, n, stream=None):
    """fme_refine_direct_device: device-resident jobs and 64-byte records (addresses or torch
    tensors), asynchronous on `stream`; a rejected batch shows in ctx.refine_status()."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_direct_device(ctx.h, _dev(d_jobs), _dev(d_res), int(n), stream))


def refine_direct_mv_device(ctx, d_jobs, d_out, n, stream=None):
    """fme_refine_direct_mv_device: the same with the 16-byte MV_RESULT_DTYPE records."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_direct_mv_device(ctx.h, _dev(d_jobs), _dev(d_out), int(n), stream))


def last_ms(ctx):
    """{phase: device ms} of the last direct batch with profiling on (LAST_MS_NAMES)."""
    lib = bind(ctx.lib)
    ms = np.zeros(4, np.float32)
    _check(lib, lib.fme_refine_direct_last_ms(ctx.h, _ptr(ms)))
    return dict(zip(LAST_MS_NAMES, ms.tolist()))


# ---- the host arithmetic of csrc/fme_direct_host.h on arrays -------------------------------------------

def _split(o):
    half = np.where(o <= -2, -1, np.where(o >= 2, 1, 0))
    return half, o - 2 * half


def half_qtr_of_class(cls):
    """(MVX_HALF, MVX_QRTER, MVY_HALF, MVY_QRTER) of a class (or an array of classes), in the order of
    fme_nn_pred_single's out4: the switch at TEncSearch.cpp:136-193."""
    cls = np.asarray(cls).astype(np.int64)
    hx, qx = _split(cls % 7 - 3)
    hy, qy = _split(cls // 7 - 3)
    return hx, qx, hy, qy


def tail_numpy(frac_cost, mv_x, mv_y, job, motion_lambda):
    """xMotionEstimation's tail (TEncSearch.cpp:4586-4597) restated for one job: (cost, bits) of the
    quarter-pel MV whose sub-pel cost is frac_cost; double arithmetic, the (UInt)(Int64) conversion."""
    mvb = _eg_bits(int(mv_x) - int(job["mvp_x"])) + _eg_bits(int(mv_y) - int(job["mvp_y"]))
    bits = int(job["bits_in"]) + mvb
    fw = 0.5 if int(job["flags"]) & JOB_BIPRED else 1.0
    val = math.floor(fw * (float(int(frac_cost)) - float(mv_cost_numpy(motion_lambda, mvb)))) + float(
        mv_cost_numpy(motion_lambda, bits))
    return int(val) & 0xFFFFFFFF, bits


def direct_numpy(jobs, results, surfaces, lambdas):
    """The records a direct batch must give for `jobs` (RESULT_DTYPE[n]): results = an ordinary
    refinement's records of the same job stream and incoming NN state (their mv_int, c, emi, n_emi,
    nn_class and status bits carry over), surfaces = the cost surfaces centred on those records' mv_int
    (surface.jobs_at_results), lambdas = what fme_set_lambda was given per id."""
    jobs = np.asarray(jobs)
    out = np.array(results, dtype=RESULT_DTYPE, copy=True)
    cost = _cost_rows(surfaces)
    n = len(out)
    cls = out["nn_class"].astype(np.int64)
    if n and int(cls.max()) >= POINTS:
        raise ValueError("direct_numpy: a record without a class (nn_mode 0)")
    hx, qx, hy, qy = half_qtr_of_class(cls)
    out["half_x"], out["qtr_x"], out["half_y"], out["qtr_y"] = hx, qx, hy, qy
    mvx = 4 * out["mv_int_x"].astype(np.int64) + cls % 7 - 3
    mvy = 4 * out["mv_int_y"].astype(np.int64) + cls // 7 - 3
    out["mv_x"], out["mv_y"] = mvx, mvy
    out["frac_cost"] = cost[np.arange(n), cls]
    for i in range(n):
        ml = 65536.0 * math.sqrt(float(lambdas[int(jobs[i]["lambda_id"])]))
        out["cost"][i], out["bits"][i] = tail_numpy(out["frac_cost"][i], mvx[i], mvy[i], jobs[i], ml)
    out["status"] = out["status"] | RES_NN_DIRECT
    return out


def mv_records(results):
    """The MV_RESULT_DTYPE view of full records (what the compact form returns)."""
    out = np.zeros(len(results), MV_RESULT_DTYPE)
    for f in ("mv_x", "mv_y", "cost", "bits", "nn_class", "status"):
        out[f] = results[f]
    return out
