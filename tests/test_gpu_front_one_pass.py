"""The batch front end in one pass (k_front): every workgroup classifies its 1,024 jobs, ranks them
per class, takes its place in each class with one atomic and writes perm at once (class c's region
starts at c * capacity); the workgroup that finishes last builds the Schedule and blk_prefix from
the other workgroups' counters and zeroes the next batch's counter block.

Results are checked against the CPU oracle, field for field, on 416x240 pictures with nn_mode 1;
perm and the Schedule are read back through fme_debug_front (a debugging export of the library that
include/fme.h does not declare)."""
import ctypes as C

import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import (JOB_BIPRED, JOB_DTYPE, MV_FIELDS, MV_RESULT_DTYPE, RES_REJECTED, RESULT_DTYPE, compare_results)

pytestmark = pytest.mark.gpu

W, H = 416, 240
QP = 22
BLOCK = 1024                      # jobs per k_front workgroup (kJobsPerScanBlock)
# one wave, one workgroup, each +-1; five workgroups with a one-job last one; 20 workgroups: more than
# one per XCD, so the last workgroup reads counters that workgroups on other XCDs wrote
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 20001)
# fme_device.h kClassW / kClassH: class id -> PU shape
CLASS_W = (4, 8, 8, 4, 16, 8, 16, 12, 16, 16, 8, 32, 16, 32, 24, 32, 32, 16, 64, 32, 64, 48, 64, 64)
CLASS_H = (8, 4, 8, 16, 4, 16, 8, 16, 12, 16, 32, 8, 32, 16, 32, 24, 32, 64, 16, 64, 32, 64, 48, 64)
NCLS = 24
SCHED_WORDS = 25 + 24 + 24 + 8 * 25 + 1   # prefix, class_off, class_cnt, xq, invalid

_PICS = {}


def _pics():
    if not _PICS:
        _PICS.update({i: synth.synth_luma(W, H, i) for i in range(5)})
    return _PICS


def _bind(eng):
    for k, v in _pics().items():
        eng.set_picture(k, v)
    for lid, lam in enumerate(synth.LDP_LAMBDA[QP]):
        eng.set_lambda(lid, lam)


def _make_ctx(**kw):
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=1, qp=QP, **kw)
    _bind(ctx)
    return ctx


def _make_oracle():
    from oracle import Oracle
    o = Oracle(nn_mode=1, qp=QP)
    _bind(o)
    o.load_nn(weights.load_weights(QP))
    return o


_CTX = []


def _ctx():
    """One context for the tests that leave it as they found it (max_jobs 0: perm grows with the batches)."""
    if not _CTX:
        _CTX.append(_make_ctx())
    return _CTX[0]


def _jobs(n, seed, shapes=None):
    """n jobs; without `shapes` the first 24 are the 24 PU shapes and the rest follow the usual mix."""
    rng = np.random.default_rng(seed)
    if shapes is None:
        w, h = synth.sample_sizes(rng, n)
        k = min(n, len(synth.ALL_PU_SIZES))
        w[:k] = [s[0] for s in synth.ALL_PU_SIZES[:k]]
        h[:k] = [s[1] for s in synth.ALL_PU_SIZES[:k]]
    else:
        pick = rng.integers(0, len(shapes), n)
        w = np.array([s[0] for s in shapes], np.int32)[pick]
        h = np.array([s[1] for s in shapes], np.int32)[pick]
    return synth.make_jobs(rng, W, H, n, 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(w, h))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _canonical(jobs):
    from nnfme.runtime import pack_jobs, unpack_jobs
    pk, kb = pack_jobs(jobs)
    return pk, kb, unpack_jobs(pk, kb)


def _issue(ctx, jobs, packed, mv=False):
    """Enqueues one batch (no host synchronisation); returns the device output and what keeps the inputs alive."""
    import torch
    pk, kb, uj = _canonical(jobs)
    n = len(jobs)
    dt = MV_RESULT_DTYPE if mv else RESULT_DTYPE
    d = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if packed:
        dpk, dkb = _dev(pk), _dev(kb)
        fn = ctx.refine_mv_packed_device if mv else ctx.refine_packed_device
        fn(dpk.data_ptr(), dkb.data_ptr(), d.data_ptr(), n, s)
        keep = (dpk, dkb)
    else:
        duj = _dev(uj)
        fn = ctx.refine_mv_device if mv else ctx.refine_device
        fn(duj.data_ptr(), d.data_ptr(), n, s)
        keep = (duj,)
    return d, dt, keep


def _run(ctx, jobs, packed, mv=False):
    d, dt, _keep = _issue(ctx, jobs, packed, mv)
    status = ctx.refine_status()
    return d.cpu().numpy().view(dt), status


def _check_full(got, want, what):
    bad, first, counts = compare_results(got, want)            # every field; emi: the n_emi pushed values
    assert bad == 0, f"{what}: {bad} jobs differ from the oracle, first {first}: {counts}"
    assert np.array_equal(got["status"], want["status"]), f"{what}: status differs from the oracle"


def _check_mv(got, want, what):
    for f in MV_FIELDS:
        assert np.array_equal(got[f], want[f]), f"{what}: fme_mv_result.{f} differs from the oracle"


def _check_batch(ctx, jobs, want, what):
    """The batch as packed and as unpacked rows, full records and fme_mv_result, each from a reset NN state."""
    for packed in (True, False):
        for mv in (False, True):
            ctx.nn_reset()
            got, status = _run(ctx, jobs, packed, mv)
            assert status == 0, what
            (_check_mv if mv else _check_full)(got, want, f"{what} {'packed' if packed else 'unpacked'}")


_WANT = {}


def _oracle_results(key, jobs):
    """Computed once per batch and left unchanged."""
    if key not in _WANT:
        _WANT[key] = _make_oracle().refine(_canonical(jobs)[2])
    return _WANT[key]


# ---- workgroup seams -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_seams_all_shapes(n):
    jobs = _jobs(n, 500 + n)
    if n >= 64:
        assert len(set(zip(jobs["w"].tolist(), jobs["h"].tolist()))) == 24
    _check_batch(_ctx(), jobs, _oracle_results(("all", n), jobs), f"n={n}")


def test_two_shapes_leave_22_classes_empty():
    jobs = _jobs(2500, 61, shapes=[(8, 8), (32, 16)])
    _check_batch(_ctx(), jobs, _oracle_results("two", jobs), "two shapes")


def test_single_64x64_job_last():
    n = 2 * BLOCK + 1                                     # the job is alone in the last workgroup
    jobs = _jobs(n, 62, shapes=[(4, 8), (8, 4), (8, 8), (16, 16)])
    last = synth.make_jobs(np.random.default_rng(63), W, H, 1, 4, [2], [1], sizes=([64], [64]))
    jobs[n - 1] = last[0]
    assert ((jobs["w"] == 64) & (jobs["h"] == 64)).sum() == 1
    _check_batch(_ctx(), jobs, _oracle_results("one64", jobs), "single 64x64 job")


# ---- perm and the Schedule -------------------------------------------------------------------------
def _debug_front(ctx, cap_only=False):
    fn = ctx.lib.fme_debug_front
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
    cap = C.c_int32(0)
    assert fn(ctx.h, None, 0, None, 0, C.byref(cap)) == 0
    if cap_only:
        return cap.value
    perm = np.zeros(NCLS * cap.value, np.int32)
    sched = np.zeros(SCHED_WORDS, np.int32)
    assert fn(ctx.h, perm.ctypes.data, perm.size, sched.ctypes.data, sched.size, None) == 0
    return cap.value, perm, sched


def _lanes_per_pu(c):
    """fme_lane.hip lane_lanes_per_pu: 4x8 units (4x4 for PUs 4 or 12 high), halved above 64, rounded up to a power of two."""
    w, h = CLASS_W[c], CLASS_H[c]
    u = (w // 4) * (h // (4 if h in (4, 12) else 8))
    if u > 64:
        u //= 2
    return 1 << (u - 1).bit_length()


def test_perm_is_a_permutation_by_class():
    n = 20001
    jobs = _jobs(n, 500 + n)
    ctx = _ctx()
    ctx.nn_reset()
    _got, status = _run(ctx, jobs, packed=True)
    assert status == 0
    cap, perm, sched = _debug_front(ctx)
    assert cap >= n
    prefix, class_off, class_cnt = sched[0:25], sched[25:49], sched[49:73]
    xq, invalid = sched[73:273].reshape(8, 25), sched[273]
    lut = {(CLASS_W[c], CLASS_H[c]): c for c in range(NCLS)}
    cls = np.array([lut[wh] for wh in zip(jobs["w"].tolist(), jobs["h"].tolist())])
    assert invalid == 0
    assert np.array_equal(class_cnt, np.bincount(cls, minlength=NCLS))
    assert np.array_equal(class_off, np.arange(NCLS) * cap)
    for c in range(NCLS):
        region = perm[c * cap: c * cap + class_cnt[c]]
        assert np.array_equal(np.sort(region), np.flatnonzero(cls == c)), f"class {c}: not its jobs, each once"
        # a workgroup's jobs of a class sit together, in call order
        blk = region // BLOCK
        starts = np.flatnonzero(np.diff(blk, prepend=-1) != 0)
        assert len(starts) == len(set(blk.tolist())), f"class {c}: a workgroup's jobs are split"
        same = np.diff(blk) == 0
        assert np.all(np.diff(region)[same] > 0), f"class {c}: indices of one workgroup do not ascend"
    # the wave tiles and the per-XCD queues, restated from class_cnt (lane_class_at: class order)
    nb = np.array([(int(class_cnt[c]) * _lanes_per_pu(c) + 63) // 64 for c in range(NCLS)], np.int64)
    assert np.array_equal(prefix, np.concatenate([[0], np.cumsum(nb)]))
    for x in range(8):
        band = nb * (x + 1) // 8 - nb * x // 8
        assert np.array_equal(xq[x], np.concatenate([[0], np.cumsum(band)])), f"xq[{x}]"


# ---- rejection -------------------------------------------------------------------------------------
def _spoil(jobs, at, how):
    bad = jobs.copy()
    if how == "shape":
        bad["w"][at], bad["h"][at] = 20, 20            # on the 4x4 grid, but no HEVC inter PU shape
        bad["x"][at], bad["y"][at] = 0, 0
    else:
        bad["ref_id"][at] = 40                         # an unset picture slot
    return bad


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("how", ["shape", "slot"])
@pytest.mark.parametrize("where", ["last", "first"])
def test_one_invalid_job_rejects_the_batch(where, how, packed):
    n = 3 * BLOCK                                       # the last job of the last workgroup is job n - 1
    ctx = _ctx()
    ctx.nn_reset()
    _run(ctx, _jobs(300, 70), packed=True)              # some NN state to keep
    before = ctx.nn_get_state()
    bad = _spoil(_jobs(n, 71), n - 1 if where == "last" else 0, how)
    got, status = _run(ctx, bad, packed)
    assert status == 1
    assert np.all(got["status"] == RES_REJECTED)
    assert np.array_equal(ctx.nn_get_state(), before)


# ---- the counter blocks alternate ------------------------------------------------------------------
def test_counters_after_rejection_and_integer_search():
    import torch
    ctx = _make_ctx()
    orc = _make_oracle()
    s = torch.cuda.current_stream()
    bad = _spoil(_jobs(1500, 80), 1499, "slot")
    good = _jobs(2300, 81)
    ctx.nn_reset()
    d_bad, _, keep_bad = _issue(ctx, bad, packed=True)      # no host synchronisation between the two
    d_good, _, keep_good = _issue(ctx, good, packed=True)
    assert ctx.refine_status() == 0
    assert np.all(d_bad.cpu().numpy().view(RESULT_DTYPE)["status"] == RES_REJECTED)
    _check_full(d_good.cpu().numpy().view(RESULT_DTYPE), orc.refine(_canonical(good)[2]), "after a rejected batch")
    # once more, so that both counter blocks have been counted in and zeroed by a k_front
    third = _jobs(900, 82)
    got, status = _run(ctx, third, packed=False)
    assert status == 0
    _check_full(got, orc.refine(_canonical(third)[2]), "third batch")
    # an integer search marks the counter blocks dirty; the next batch fills them first
    tz_jobs, ext = synth.make_tz_jobs(np.random.default_rng(83), W, H, 3, 4, [0, 1, 2, 3], [0, 1, 2, 3], search_range=8)
    dj, de = _dev(tz_jobs), _dev(ext)
    ds = torch.zeros(len(tz_jobs), dtype=torch.int32, device="cuda")
    ctx.integer_search_device(dj.data_ptr(), de.data_ptr(), ds.data_ptr(), len(tz_jobs), s.cuda_stream)
    s.synchronize()
    got_tz = dj.cpu().numpy().view(JOB_DTYPE)
    exp_tz, exp_sad = orc.integer_search(tz_jobs, ext)
    assert np.array_equal(got_tz["mv_x"], exp_tz["mv_x"]) and np.array_equal(got_tz["mv_y"], exp_tz["mv_y"])
    assert np.array_equal(ds.cpu().numpy().view(np.uint32), exp_sad)
    for k, nn in enumerate((1300, 2100)):
        jobs = _jobs(nn, 84 + k)
        got, status = _run(ctx, jobs, packed=True)
        assert status == 0
        _check_full(got, orc.refine(_canonical(jobs)[2]), f"batch {k} after an integer search")
    del keep_bad, keep_good


# ---- keyed packed groups across a workgroup seam ---------------------------------------------------
def test_keyed_jobs_across_a_workgroup_seam():
    n = BLOCK + 80
    jobs = _jobs(n, 90)
    keyed = list(range(1020, 1031))                     # the 64-job groups 15 and 16: two workgroups
    jobs["flags"][keyed] = JOB_BIPRED
    jobs["key_offset"][keyed] = -2
    reqs, key_count = synth.make_bipred_key_reqs(np.random.default_rng(91), jobs, 4, [0, 1, 2, 3])
    keys = synth.bipred_keys(reqs, _pics(), key_count)
    _pk, kb, uj = _canonical(jobs)
    assert kb[15] == 0 and kb[16] > 0 and np.all(np.delete(kb, [15, 16]) == -1)
    assert np.array_equal(uj["key_offset"], jobs["key_offset"])
    ctx = _make_ctx()
    orc = _make_oracle()
    ctx.set_keys(keys)
    orc.set_keys(keys)
    _check_batch(ctx, jobs, orc.refine(uj), "keyed across a seam")
