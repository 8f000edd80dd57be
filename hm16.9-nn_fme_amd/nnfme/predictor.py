"""An external sub-pel predictor (include/fme_extern.h) over libfme_amd.so: the NN inputs of every
job out as device rows, one class per job in from a device array.

The ctypes prototypes of the header's entry points (additional exports, bound on the handle
runtime.load_library() returns) with wrappers that raise FmeError; the rows and the records those
entry points must produce restated in numpy (rows_numpy on dataset.nn_inputs, refine_at_numpy on
direct.direct_numpy); the rows as the float32 features SSE.csv names, on the host and as a torch
tensor on the device; and run(), which chains inputs -> features -> model -> evaluation on one
stream.  There is no CPU fallback: a library without these symbols raises FmeError.
"""
import ctypes as C

import numpy as np

from . import dataset, direct
from .abi import JOB_DTYPE, JOB_EMI, RES_NN_STALE, RES_NN_UNINIT, RES_REJECTED, RESULT_DTYPE
from .runtime import FmeError, _check, _ptr
from .surface import POINTS

RES_NN_EXTERN = 0x08
LAST_MS_NAMES = ("emi", "rows", "evaluation", "batch")

# fme_nn_row
NN_ROW_DTYPE = np.dtype([("e", "<u4", (8,)), ("c", "<u4"), ("pu_h", "<u4"), ("pu_w", "<u4"),
                         ("mv_int_x", "<i2"), ("mv_int_y", "<i2"), ("n_emi", "u1"), ("writes", "u1"),
                         ("status", "<u2"), ("reserved", "<u4", (3,))])
assert NN_ROW_DTYPE.itemsize == 64

# The functions include/fme_extern.h declares.
EXTERN_SYMBOLS = ("fme_nn_inputs", "fme_nn_inputs_device", "fme_refine_at", "fme_refine_at_device",
                  "fme_refine_at_mv_device", "fme_refine_at_status", "fme_extern_last_ms")

# The row's 32-bit words in SSE.csv column order: top_left .. bottom_right (dataset.CONT_VARS, C in
# the middle), then Height, then Width.
FEATURE_WORDS = (0, 1, 2, 3, 8, 4, 5, 6, 7, 9, 10)


def bind(lib):
    """Set the prototypes of the fme_extern.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_extern_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_nn_inputs": (I, [P, P, P, I, P]),
        "fme_nn_inputs_device": (I, [P, P, P, I, P]),
        "fme_refine_at": (I, [P, P, P, P, P, I, P]),
        "fme_refine_at_device": (I, [P, P, P, P, P, I, P]),
        "fme_refine_at_mv_device": (I, [P, P, P, P, P, I, P]),
        "fme_refine_at_status": (I, [P]),
        "fme_extern_last_ms": (I, [P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_extern.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_extern_bound = True
    return lib


_dev = direct._dev


def nn_inputs(ctx, jobs, stream=None):
    """fme_nn_inputs on host arrays: NN_ROW_DTYPE[n]; the context's NN state advances."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    rows = np.zeros(len(jobs), dtype=NN_ROW_DTYPE)
    _check(lib, lib.fme_nn_inputs(ctx.h, _ptr(jobs), _ptr(rows), len(jobs), stream))
    return rows


def nn_inputs_device(ctx, d_jobs, d_rows, n, stream=None):
    """fme_nn_inputs_device: device-resident jobs and 64-byte rows (addresses or torch tensors),
    asynchronous on `stream`; a rejected batch shows in ctx.refine_status()."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_nn_inputs_device(ctx.h, _dev(d_jobs), _dev(d_rows), int(n), stream))


def refine_at(ctx, jobs, classes, rows=None, stream=None, out=None):
    """fme_refine_at on host arrays: RESULT_DTYPE[n] (written into `out` when given)."""
    lib = bind(ctx.lib)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    cls = np.ascontiguousarray(classes, dtype=np.uint8)
    if len(cls) != len(jobs) or (rows is not None and len(rows) != len(jobs)):
        raise ValueError("refine_at: one class (and one row) per job")
    r = None if rows is None else np.ascontiguousarray(rows, dtype=NN_ROW_DTYPE)
    res = np.zeros(len(jobs), dtype=RESULT_DTYPE) if out is None else out
    _check(lib, lib.fme_refine_at(ctx.h, _ptr(jobs), None if r is None else _ptr(r), _ptr(cls), _ptr(res),
                                  len(jobs), stream))
    return res


def refine_at_device(ctx, d_jobs, d_rows, d_cls, d_res, n, stream=None):
    """fme_refine_at_device: d_rows may be None (the EMI step runs)."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_at_device(ctx.h, _dev(d_jobs), _dev(d_rows), _dev(d_cls), _dev(d_res), int(n), stream))


def refine_at_mv_device(ctx, d_jobs, d_rows, d_cls, d_out, n, stream=None):
    """fme_refine_at_mv_device: the same with the 16-byte MV_RESULT_DTYPE records."""
    lib = bind(ctx.lib)
    _check(lib, lib.fme_refine_at_mv_device(ctx.h, _dev(d_jobs), _dev(d_rows), _dev(d_cls), _dev(d_out), int(n), stream))


def refine_at_status(ctx):
    """Jobs the last refine_at batch refused one by one (waits for it)."""
    lib = bind(ctx.lib)
    rc = lib.fme_refine_at_status(ctx.h)
    if rc < 0:
        _check(lib, rc)
    return rc


def last_ms(ctx):
    """{phase: device ms} of the last call of either family with profiling on (LAST_MS_NAMES)."""
    lib = bind(ctx.lib)
    ms = np.zeros(4, np.float32)
    _check(lib, lib.fme_extern_last_ms(ctx.h, _ptr(ms)))
    return dict(zip(LAST_MS_NAMES, ms.tolist()))


# ---- the rows and the records restated in numpy --------------------------------------------------------

def rows_numpy(jobs, results, state_in=None, slot_reset=False):
    """(rows NN_ROW_DTYPE[n], state_out uint32[12]): what fme_nn_inputs must give for `jobs`, from an
    ordinary refinement's records of the same job stream (their emi, n_emi, c, mv_int) and the NN
    state carried into the batch.  slot_reset: the rule of a net with FME_NN_IN_SLOT_RESET (a slot the
    job did not push itself reads 0)."""
    jobs = np.asarray(jobs)
    n = len(jobs)
    st = np.zeros(12, np.uint32) if state_in is None else np.asarray(state_in, np.uint32).reshape(12)
    e, c, pu_h, pu_w, out = dataset.nn_inputs(jobs, results, st)
    emi_job = (jobs["flags"] & JOB_EMI) != 0
    n_emi = np.asarray(results["n_emi"]).astype(np.int64)
    own = emi_job[:, None] & (n_emi[:, None] > np.arange(8)[None, :])
    # which carried fields had a writer at or before each job (or in the state carried in)
    seen = np.zeros((n, 9), bool)
    seen[:, :8] = np.logical_or.accumulate(own, axis=0) if n else own
    seen[:, 8] = np.logical_or.accumulate(emi_job) if n else emi_job
    seen |= ((int(st[11]) >> np.arange(9)) & 1).astype(bool)[None, :]
    if slot_reset:
        e = np.where(own, np.asarray(results["emi"]), 0).astype(np.uint32)
        seen[:, :8] = True
        if n:
            out[:8] = e[-1]
            out[11] |= 0xFF
    rows = np.zeros(n, NN_ROW_DTYPE)
    rows["e"], rows["c"], rows["pu_h"], rows["pu_w"] = e, c, pu_h, pu_w
    rows["mv_int_x"], rows["mv_int_y"] = results["mv_int_x"], results["mv_int_y"]
    rows["n_emi"] = results["n_emi"]
    rows["writes"] = emi_job
    rows["status"] = (np.where(~emi_job | (n_emi < 8), RES_NN_STALE, 0) |
                      np.where(~seen.all(axis=1), RES_NN_UNINIT, 0))
    return rows, out


def records_of_rows(rows):
    """The EMI fields of the records fme_refine_at builds from rows (csrc/fme_extern_host.h
    extern_row_record): mv_int, n_emi, emi[s] = e[s] for s < n_emi, c where `writes`; all else 0."""
    rows = np.asarray(rows)
    out = np.zeros(len(rows), RESULT_DTYPE)
    n_emi = np.minimum(rows["n_emi"], 8)
    out["mv_int_x"], out["mv_int_y"], out["n_emi"] = rows["mv_int_x"], rows["mv_int_y"], n_emi
    out["emi"] = np.where(n_emi[:, None] > np.arange(8)[None, :], rows["e"], 0)
    out["c"] = np.where(rows["writes"] != 0, rows["c"], 0)
    return out


def refine_at_numpy(jobs, results, classes, surfaces, lambdas):
    """The records fme_refine_at must give (RESULT_DTYPE[n]): direct.direct_numpy on a copy of
    `results` (an ordinary refinement's records, or records_of_rows) whose nn_class is replaced by
    `classes`; status is RES_NN_DIRECT | RES_NN_EXTERN; a class above 48 refuses its job alone (the
    record 0 but for RES_REJECTED)."""
    cls = np.asarray(classes).astype(np.int64).reshape(-1)
    res = np.array(results, dtype=RESULT_DTYPE, copy=True)
    if len(cls) != len(res):
        raise ValueError("refine_at_numpy: one class per job")
    refused = (cls < 0) | (cls >= POINTS)
    res["nn_class"] = np.where(refused, 24, cls)
    out = direct.direct_numpy(jobs, res, surfaces, lambdas)
    out["status"] = direct.RES_NN_DIRECT | RES_NN_EXTERN
    if refused.any():
        blank = np.zeros(1, RESULT_DTYPE)
        blank["status"] = RES_REJECTED
        out[refused] = blank[0]
    return out


# ---- the rows as model inputs ---------------------------------------------------------------------------

def features(rows):
    """float32 [n, 11] in SSE.csv column order: the nine distortions as dataset.CONT_VARS (top_left,
    top_center, top_right, left, center = C, right, bottom_left, bottom_center, bottom_right), then
    Height, then Width."""
    w = np.ascontiguousarray(rows, dtype=NN_ROW_DTYPE).view("<u4").reshape(-1, 16)
    return w[:, list(FEATURE_WORDS)].astype(np.float32)


def rows_torch(d_rows):
    """A device tensor of rows (any dtype, 64 bytes per row) as its int32 words [n, 16], no copy."""
    import torch
    return d_rows.contiguous().view(torch.uint8).reshape(-1).view(torch.int32).reshape(-1, 16)


def features_torch(d_rows):
    """features() of a device tensor of rows, on its device: float32 [n, 11]."""
    import torch
    w = rows_torch(d_rows)
    # FEATURE_WORDS as slices (an index tensor would have to be uploaded first)
    cols = torch.cat([w[:, 0:4], w[:, 8:9], w[:, 4:8], w[:, 9:11]], dim=1)
    # the words are unsigned: through int64, so that a distortion of 2^31 or more stays positive
    return (cols.to(torch.int64) & 0xFFFFFFFF).to(torch.float32)


def run(ctx, d_jobs, model, d_rows, d_cls, d_res, stream=None, topk=None):
    """One stream-ordered step with any torch predictor, nothing synchronised: the inputs call,
    features_torch, `model` with its argmax to uint8 into d_cls, fme_refine_at_device with the rows.

    d_jobs: uint8 tensor of JOB_DTYPE records; d_rows (64 n bytes), d_cls (uint8 [n]) and d_res (64 n
    bytes) are the caller's device tensors; stream: a torch.cuda.Stream (None: the current one).
    model(x) returns scores [n, 49] (their argmax is the class) or the classes [n] themselves; a model
    with a true attribute `takes_rows` gets the rows' int32 words [n, 16] instead of the features.

    topk = k (1..8): the model returns scores [n, 49], d_cls is uint8 [n, k] and receives the scores'
    topk(k) indices as each job's candidate list, and fme_refine_among_device (include/fme_among.h)
    runs on it instead: the record is the best of the k."""
    import torch
    n = int(d_cls.numel()) if topk is None else int(d_cls.numel()) // int(topk)
    stream = torch.cuda.current_stream(d_cls.device) if stream is None else stream
    with torch.cuda.stream(stream):
        nn_inputs_device(ctx, d_jobs, d_rows, n, stream.cuda_stream)
        x = rows_torch(d_rows) if getattr(model, "takes_rows", False) else features_torch(d_rows)
        with torch.no_grad():
            y = model(x)
        if topk is None:
            d_cls.copy_((y.argmax(dim=1) if y.dim() == 2 else y).to(torch.uint8))
            refine_at_device(ctx, d_jobs, d_rows, d_cls, d_res, n, stream.cuda_stream)
        else:
            from . import among
            if y.dim() != 2:
                raise ValueError("run(topk=k): the model returns scores [n, 49]")
            d_cls.view(n, int(topk)).copy_(y.topk(int(topk), dim=1).indices.to(torch.uint8))
            among.refine_among_device(ctx, d_jobs, d_rows, d_cls, int(topk), d_res, None, n, stream.cuda_stream)

