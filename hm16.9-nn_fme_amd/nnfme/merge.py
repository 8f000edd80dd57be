"""Prediction error and merge estimation (include/fme_merge.h) over libfme_amd.so.

The numpy mirrors of fme_pe_task / fme_merge_req / fme_merge_res, the ctypes prototypes of the
header's entry points (bound on the handle runtime.load_library() returns; they are additional
exports, not part of runtime.ABI_SYMBOLS), and wrappers that raise FmeError with the library's
code.  There is no CPU fallback: a library without these symbols raises FmeError.
"""
import ctypes as C

import numpy as np

from .runtime import FmeError, _check, _ptr

PE_LOSSLESS = 0x04
MRG_HAS_ME = 0x08
MRG_MAX_CAND = 5
NO_COST = 0xFFFFFFFF

PE_TASK_DTYPE = np.dtype([
    ("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("org_id", "u1"), ("flags", "u1"),
    ("cu_x", "<u2"), ("cu_y", "<u2"), ("ref_id", "u1", (2,)), ("reserved", "<u2"), ("mv", "<i2", (2, 2)),
])
assert PE_TASK_DTYPE.itemsize == 24

MERGE_CAND_DTYPE = np.dtype([
    ("inter_dir", "u1"), ("ref_id", "u1", (2,)), ("reserved", "u1"), ("mv", "<i2", (2, 2)),
])
assert MERGE_CAND_DTYPE.itemsize == 12

MERGE_REQ_DTYPE = np.dtype([
    ("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("org_id", "u1"), ("lambda_id", "u1"),
    ("cu_x", "<u2"), ("cu_y", "<u2"), ("cu_w", "u1"), ("max_num_merge_cand", "u1"), ("n_cand", "u1"), ("flags", "u1"),
    ("cand", MERGE_CAND_DTYPE, (MRG_MAX_CAND,)),
    ("me_inter_dir", "u1"), ("me_ref_id", "u1", (2,)), ("reserved", "u1"), ("me_mv", "<i2", (2, 2)),
    ("me_bits", "<u4"), ("reserved2", "<u4"),
])
assert MERGE_REQ_DTYPE.itemsize == 96

MERGE_RES_DTYPE = np.dtype([
    ("use_merge", "u1"), ("merge_idx", "u1"), ("merge_inter_dir", "u1"), ("inter_dir", "u1"),
    ("ref_id", "u1", (2,)), ("reserved", "<u2"), ("mv", "<i2", (2, 2)),
    ("merge_cost", "<u4"), ("cand_dist", "<u4", (MRG_MAX_CAND,)), ("cand_cost", "<u4", (MRG_MAX_CAND,)),
    ("me_dist", "<u4"), ("me_cost", "<u4"), ("cost", "<u4"),
])
assert MERGE_RES_DTYPE.itemsize == 72

# The functions include/fme_merge.h declares (tests/test_merge_abi.py checks the header against this).
MERGE_SYMBOLS = ("fme_pred_error", "fme_pred_error_device", "fme_pred_error_invalid_count",
                 "fme_pred_error_last_ms", "fme_merge_estimate")


def bind(lib):
    """Set the prototypes of the fme_merge.h entry points on a loaded library (once)."""
    if getattr(lib, "_fme_merge_bound", False):
        return lib
    P, I = C.c_void_p, C.c_int
    sig = {
        "fme_pred_error": (I, [P, P, P, I, P]),
        "fme_pred_error_device": (I, [P, P, P, I, P]),
        "fme_pred_error_invalid_count": (I, [P]),
        "fme_pred_error_last_ms": (I, [P, P]),
        "fme_merge_estimate": (I, [P, P, P, I, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None:
            raise FmeError(-1, f"the library does not export {name} (include/fme_merge.h)")
        f.restype = res
        f.argtypes = args
    lib._fme_merge_bound = True
    return lib


def pred_error(ctx, tasks, stream=None):
    """fme_pred_error: the distortion (uint32) of every PE_TASK_DTYPE task, host arrays."""
    lib = bind(ctx.lib)
    tasks = np.ascontiguousarray(tasks, dtype=PE_TASK_DTYPE)
    dist = np.zeros(len(tasks), np.uint32)
    _check(lib, lib.fme_pred_error(ctx.h, _ptr(tasks), _ptr(dist), len(tasks), stream))
    return dist


def pred_error_device(ctx, d_tasks, d_dist, n=None, stream=None):
    """fme_pred_error_device on torch tensors: d_tasks a uint8 device tensor holding n
    PE_TASK_DTYPE records, d_dist an int32 / uint32-sized device tensor of at least n elements
    (written in stream order; an invalid task's slot is 0xFFFFFFFF).  No host synchronisation."""
    lib = bind(ctx.lib)
    if n is None:
        n = d_tasks.numel() * d_tasks.element_size() // PE_TASK_DTYPE.itemsize
    if d_tasks.numel() * d_tasks.element_size() < n * PE_TASK_DTYPE.itemsize or \
            d_dist.numel() * d_dist.element_size() < 4 * n:
        raise FmeError(-1, "pred_error_device: tensors shorter than n tasks")
    _check(lib, lib.fme_pred_error_device(ctx.h, C.c_void_p(d_tasks.data_ptr()), C.c_void_p(d_dist.data_ptr()), int(n),
                                          stream))


def pred_error_invalid_count(ctx):
    lib = bind(ctx.lib)
    rc = lib.fme_pred_error_invalid_count(ctx.h)
    if rc < 0:
        _check(lib, rc)
    return rc


def pred_error_last_ms(ctx):
    lib = bind(ctx.lib)
    ms = C.c_float()
    _check(lib, lib.fme_pred_error_last_ms(ctx.h, C.byref(ms)))
    return ms.value


def merge_estimate(ctx, reqs, stream=None):
    """fme_merge_estimate: one MERGE_RES_DTYPE record per MERGE_REQ_DTYPE request."""
    lib = bind(ctx.lib)
    reqs = np.ascontiguousarray(reqs, dtype=MERGE_REQ_DTYPE)
    res = np.zeros(len(reqs), MERGE_RES_DTYPE)
    _check(lib, lib.fme_merge_estimate(ctx.h, _ptr(reqs), _ptr(res), len(reqs), stream))
    return res


# ---- plain restatements (the fixtures' generator and the CPU tests) --------------------------------

def _had(n):
    h = np.array([[1]], np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


_H4, _H8 = _had(4), _had(8)


def dist_numpy(org, pred, hadamard, bit_depth=8):
    """setDistParam(..., bHadamard) + DistFunc on one PU (TComRdCost.cpp:277-290): xGetHADs
    (1428-1494: 8x8 Hadamards when both sides are multiples of 8, else 4x4) or the full SAD, the
    PU's sum shifted right by bit_depth - 8."""
    d = np.asarray(org, np.int64) - np.asarray(pred, np.int64)
    h, w = d.shape
    if not hadamard:
        s = int(np.abs(d).sum())
    elif w % 8 == 0 and h % 8 == 0:
        b = d.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        s = int(((np.abs(_H8 @ b @ _H8).sum(axis=(2, 3)) + 2) >> 2).sum())
    else:
        b = d.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3)
        s = int(((np.abs(_H4 @ b @ _H4).sum(axis=(2, 3)) + 1) >> 1).sum())
    return s >> (bit_depth - 8)


_LUMA_TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0],
                       [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)


def predict_numpy(lumas, task, bit_depth=8):
    """The luma motionCompensation of one PE_TASK_DTYPE task (TComPrediction.cpp:476-668): clipMv
    per list, xCheckIdenticalMotion, xPredInterBlk in the two-stage form of csrc/fme_mc.hip's header
    (the identity filter at a zero fraction gives filterCopy and the 1-D filters exactly), uni-pred
    clipped to the bit depth, bi-pred through TComYuv::addAvg.  lumas: {slot: [H, W] samples}."""
    x, y, w, h = (int(task[f]) for f in ("x", "y", "w", "h"))
    lists = [l for l in range(2) if int(task["flags"]) & (1 << l)]
    if len(lists) == 2 and int(task["ref_id"][0]) == int(task["ref_id"][1]) and \
            tuple(task["mv"][0]) == tuple(task["mv"][1]):
        lists = [0]
    uni = len(lists) == 1
    half, maxv = 1 << (bit_depth - 1), (1 << bit_depth) - 1
    out = []
    for l in lists:
        pic = np.asarray(lumas[int(task["ref_id"][l])])
        ph, pw = pic.shape
        mx, my = int(task["mv"][l][0]), int(task["mv"][l][1])
        mx = min((pw + 8 - int(task["cu_x"]) - 1) << 2, max((-64 - 8 - int(task["cu_x"]) + 1) * 4, mx))
        my = min((ph + 8 - int(task["cu_y"]) - 1) << 2, max((-64 - 8 - int(task["cu_y"]) + 1) * 4, my))
        rows = np.clip(np.arange(y + (my >> 2) - 3, y + (my >> 2) + h + 4), 0, ph - 1)
        cols = np.clip(np.arange(x + (mx >> 2) - 3, x + (mx >> 2) + w + 4), 0, pw - 1)
        win = pic[np.ix_(rows, cols)].astype(np.int64) - half
        ch, cv = _LUMA_TAPS[mx & 3], _LUMA_TAPS[my & 3]
        s1 = sum(int(ch[k]) * win[:, k:k + w] for k in range(8)) >> (bit_depth - 8)
        s2 = sum(int(cv[k]) * s1[k:k + h, :] for k in range(8))
        if uni:
            sh = 20 - bit_depth
            return np.clip(((s2 + (1 << (sh - 1))) >> sh) + half, 0, maxv)
        out.append(s2 >> 6)
    sh = 15 - bit_depth
    return np.clip((out[0] + out[1] + (1 << (sh - 1)) + 2 * 8192) >> sh, 0, maxv)


def pred_error_numpy(lumas, task, use_hadamard, bit_depth=8):
    """xGetInterPredictionError of one task, restated: predict_numpy + dist_numpy."""
    x, y, w, h = (int(task[f]) for f in ("x", "y", "w", "h"))
    org = np.asarray(lumas[int(task["org_id"])])[y:y + h, x:x + w]
    had = bool(use_hadamard) and not int(task["flags"]) & PE_LOSSLESS
    return dist_numpy(org, predict_numpy(lumas, task, bit_depth), had, bit_depth)


def merge_decide_numpy(req, dist, motion_lambda):
    """TEncSearch.cpp:3625-3653 and 4126-4171 for one request: dist holds the distortions of its
    n_cand candidates (after xRestrictBipredMergeCand), then of the ME motion (MRG_HAS_ME)."""
    r = np.zeros((), MERGE_RES_DTYPE)
    r["cand_dist"] = r["cand_cost"] = NO_COST
    n = int(req["n_cand"])
    restricted = int(req["cu_w"]) == 8 and (int(req["w"]) < 8 or int(req["h"]) < 8)

    def motion(inter_dir, ref_id, mv):
        ref_id, mv = np.array(ref_id, np.uint8), np.array(mv, np.int16)
        for l in range(2):
            if not inter_dir & (1 << l):
                ref_id[l] = 0
                mv[l] = 0
        return inter_dir, ref_id, mv

    def cost_of(bits):
        return int((float(motion_lambda) * float(bits)) / 65536.0)

    mrg_cost, mrg_idx = NO_COST, 0
    for k in range(n):
        bits = k + 1 - (1 if k == int(req["max_num_merge_cand"]) - 1 else 0)
        c = (int(dist[k]) + cost_of(bits)) & 0xFFFFFFFF
        r["cand_dist"][k], r["cand_cost"][k] = dist[k], c
        if c < mrg_cost:
            mrg_cost, mrg_idx = c, k
    r["merge_cost"] = mrg_cost
    best = None
    if mrg_cost != NO_COST:
        cd = req["cand"][mrg_idx]
        d = int(cd["inter_dir"])
        best = motion(1 if (d == 3 and restricted) else d, cd["ref_id"], cd["mv"])
        r["merge_idx"], r["merge_inter_dir"] = mrg_idx, best[0]
    me_cost = NO_COST
    r["me_dist"] = NO_COST
    if int(req["flags"]) & MRG_HAS_ME:
        r["me_dist"] = dist[n]
        me_cost = (int(dist[n]) + cost_of(int(req["me_bits"]))) & 0xFFFFFFFF
    r["me_cost"] = me_cost
    use = mrg_cost < me_cost
    r["use_merge"] = int(use)
    pick = best if use else motion(int(req["me_inter_dir"]), req["me_ref_id"], req["me_mv"])
    r["inter_dir"], r["ref_id"], r["mv"] = pick
    r["cost"] = mrg_cost if use else me_cost
    return r


def cu_origin(x, y, w, h):
    """A CU origin for a PU at (x, y): the smallest square CU that holds the shape, on its grid where
    the PU then lies inside it, else placed so that the PU is its last (or first) partition.  clipMv
    keeps the prediction's reads inside HM's picture margin only for a PU inside its CU."""
    from .synth import cu_size_for
    s = cu_size_for(w, h)

    def one(p, n):
        o = p % s
        if o + n > s:
            o = s - n if p >= s - n else 0
        return p - o
    return one(int(x), int(w)), one(int(y), int(h))


def expand_requests(reqs):
    """The requests' PE_TASK_DTYPE tasks in fme_merge_estimate's order, and each request's first task."""
    tasks, first = [], []
    for q in reqs:
        first.append(len(tasks))
        restricted = int(q["cu_w"]) == 8 and (int(q["w"]) < 8 or int(q["h"]) < 8)
        motions = [(int(c["inter_dir"]), c["ref_id"], c["mv"]) for c in q["cand"][:int(q["n_cand"])]]
        motions = [((1 if (d == 3 and restricted) else d), rid, mv) for d, rid, mv in motions]
        if int(q["flags"]) & MRG_HAS_ME:
            motions.append((int(q["me_inter_dir"]), q["me_ref_id"], q["me_mv"]))
        for d, rid, mv in motions:
            t = np.zeros((), PE_TASK_DTYPE)
            for f in ("x", "y", "w", "h", "org_id", "cu_x", "cu_y"):
                t[f] = q[f]
            t["flags"] = d | (int(q["flags"]) & PE_LOSSLESS)
            for l in range(2):
                if d & (1 << l):
                    t["ref_id"][l] = rid[l]
                    t["mv"][l] = mv[l]
            tasks.append(t)
    return np.array(tasks, dtype=PE_TASK_DTYPE).reshape(-1), np.array(first, np.int64)
