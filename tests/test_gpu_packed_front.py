"""The batch front end on packed jobs read in place: fme_refine*_packed_device hand the caller's
16-byte rows to every kernel of the batch (k_front computes the keyed jobs' offsets and groups the
jobs by class; its last workgroup builds the schedule and zeroes the counters of the batch after
next), with no unpacked copy and no fill dispatch between batches.

Everything is checked against the unpacked entry points on fme_unpack_jobs(fme_pack_jobs(jobs)),
field for field, and against the CPU oracle on those jobs, on a 416x240 picture."""
import os

import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import (JOB_BIPRED, JOB_DTYPE, MV_RESULT_DTYPE, RES_REJECTED, RESULT_DTYPE, compare_results)

pytestmark = pytest.mark.gpu

W, H = 416, 240
QP = 22
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)   # one wave, one 1024-job scan block, each +-1; a third block of one job
VARIANTS = ("d8", "d10", "d10px")                  # bit depth 8; 10 with the default search; 10 with FME_MAIN10_SEARCH=px
MV_PARITY = ("mv_x", "mv_y", "cost", "bits", "nn_class")


def _depth(variant):
    return 8 if variant == "d8" else 10


_PICS = {}


def _pics(depth):
    if depth not in _PICS:
        mk = synth.synth_luma if depth == 8 else synth.synth_luma_hbd
        _PICS[depth] = {i: mk(W, H, i) for i in range(5)}
    return _PICS[depth]


def _bind(eng, depth):
    for k, v in _pics(depth).items():
        eng.set_picture(k, v)
    for lid, lam in enumerate(synth.LDP_LAMBDA[QP]):
        eng.set_lambda(lid, lam)


def _make_ctx(variant, nn_mode, **kw):
    from nnfme.runtime import FmeContext
    old = os.environ.get("FME_MAIN10_SEARCH")
    if variant == "d10px":
        os.environ["FME_MAIN10_SEARCH"] = "px"     # read once, when the context is created
    else:
        os.environ.pop("FME_MAIN10_SEARCH", None)
    try:
        ctx = FmeContext(nn_mode=nn_mode, qp=QP, bit_depth=_depth(variant), **kw)
    finally:
        if old is None:
            os.environ.pop("FME_MAIN10_SEARCH", None)
        else:
            os.environ["FME_MAIN10_SEARCH"] = old
    _bind(ctx, _depth(variant))
    return ctx


def _make_oracle(depth, nn_mode, net=None):
    from oracle import Oracle
    o = Oracle(nn_mode=nn_mode, qp=QP, bit_depth=depth)
    _bind(o, depth)
    if nn_mode == 1:
        o.load_nn(weights.load_weights(QP))
    if net is not None:
        o.load_nn_net(net)
    return o


def _jobs(n, seed):
    """n jobs; the first 24 are the 24 PU shapes and the next 16 sit at the search-range edge with
    every combination of the four range bits (15 of them push fewer than 8 EMI distortions)."""
    rng = np.random.default_rng(seed)
    w, h = synth.sample_sizes(rng, n)
    k = min(n, len(synth.ALL_PU_SIZES))
    w[:k] = [s[0] for s in synth.ALL_PU_SIZES[:k]]
    h[:k] = [s[1] for s in synth.ALL_PU_SIZES[:k]]
    jobs = synth.make_jobs(rng, W, H, n, 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(w, h))
    for b in range(16):
        i = 24 + b
        if i >= n:
            break
        jobs["lt_x"][i] = jobs["mv_x"][i] - (b & 1)
        jobs["rb_x"][i] = jobs["mv_x"][i] + ((b >> 1) & 1)
        jobs["lt_y"][i] = jobs["mv_y"][i] - ((b >> 2) & 1)
        jobs["rb_y"][i] = jobs["mv_y"][i] + ((b >> 3) & 1)
    return jobs


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _run4(ctx, jobs, reset=True):
    """The batch through the four device entry points, each from the same NN state:
    (packed full, packed mv, unpacked full, unpacked mv, the canonical jobs)."""
    import torch
    from nnfme.runtime import pack_jobs, unpack_jobs
    pk, kb = pack_jobs(jobs)
    uj = unpack_jobs(pk, kb)
    n = len(jobs)
    dpk, dkb, duj = _dev(pk), _dev(kb), _dev(uj)
    s = torch.cuda.current_stream()
    state = None if reset else ctx.nn_get_state()
    out = []
    for packed, mv in ((True, False), (True, True), (False, False), (False, True)):
        if reset:
            ctx.nn_reset()
        else:
            ctx.nn_set_state(state)
        dt = MV_RESULT_DTYPE if mv else RESULT_DTYPE
        d = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
        if packed:
            fn = ctx.refine_mv_packed_device if mv else ctx.refine_packed_device
            fn(dpk.data_ptr(), dkb.data_ptr(), d.data_ptr(), n, s.cuda_stream)
        else:
            fn = ctx.refine_mv_device if mv else ctx.refine_device
            fn(duj.data_ptr(), d.data_ptr(), n, s.cuda_stream)
        assert ctx.refine_status() == 0
        out.append(d.cpu().numpy().view(dt))
    return out[0], out[1], out[2], out[3], uj


def _check4(full_p, mv_p, full_u, mv_u, want, what):
    for f in RESULT_DTYPE.names:
        assert np.array_equal(full_p[f], full_u[f]), f"{what}: fme_result.{f} differs between packed and unpacked"
    for f in MV_RESULT_DTYPE.names:
        assert np.array_equal(mv_p[f], mv_u[f]), f"{what}: fme_mv_result.{f} differs between packed and unpacked"
    if want is None:
        return
    bad, first, counts = compare_results(full_p, want)
    assert bad == 0, f"{what}: {bad} jobs differ from the oracle, first {first}: {counts}"
    for f in MV_PARITY:
        assert np.array_equal(mv_p[f], want[f]), f"{what}: fme_mv_result.{f} differs from the oracle"
    assert np.array_equal(mv_p["status"], full_p["status"]), what


# ---- test 1: packed against unpacked and the oracle ------------------------------------------------
_CTX, _WANT = {}, {}


def _shared_ctx(variant, nn_mode):
    if (variant, nn_mode) not in _CTX:
        _CTX[variant, nn_mode] = _make_ctx(variant, nn_mode)
    return _CTX[variant, nn_mode]


def _oracle_results(depth, nn_mode, n, uj):
    """Computed once per (depth, NN mode, n): the pixel-kernel variant shares the depth-10 results."""
    if (depth, nn_mode, n) not in _WANT:
        _WANT[depth, nn_mode, n] = _make_oracle(depth, nn_mode).refine(uj)
    return _WANT[depth, nn_mode, n]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nn_mode", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_packed_equals_unpacked_and_oracle(n, nn_mode, variant):
    jobs = _jobs(n, 100 + n)
    if n >= 64:
        shapes = set(zip(jobs["w"].tolist(), jobs["h"].tolist()))
        assert len(shapes) == 24
    full_p, mv_p, full_u, mv_u, uj = _run4(_shared_ctx(variant, nn_mode), jobs)
    want = _oracle_results(_depth(variant), nn_mode, n, uj)
    if n >= 64:
        edge = want["n_emi"][24:40]
        assert (edge < 8).sum() == 15 and len(set(edge.tolist())) > 3
    _check4(full_p, mv_p, full_u, mv_u, want, f"n={n} nn_mode={nn_mode} {variant}")


# ---- test 2: keyed jobs ----------------------------------------------------------------------------
def _keyed_jobs():
    """Five 64-job groups: none keyed; lanes 0 and 63 keyed; three keyed in between; every second
    job keyed; a last partial group whose last job is keyed."""
    n = 4 * 64 + 20
    jobs = _jobs(n, 7)
    keyed = [64, 127, 130, 150, 171] + list(range(192, 256, 2)) + [n - 7, n - 1]
    jobs["flags"][keyed] = JOB_BIPRED
    jobs["key_offset"][keyed] = -2
    reqs, key_count = synth.make_bipred_key_reqs(np.random.default_rng(8), jobs, 4, [0, 1, 2, 3])
    keys = synth.bipred_keys(reqs, _pics(8), key_count)
    last = jobs[n - 1]
    assert int(last["key_offset"]) + int(last["w"]) * int(last["h"]) == key_count == len(keys)
    return jobs, keys


@pytest.mark.parametrize("variant", ["d8", "d10"])
def test_keyed_jobs_offsets_from_key_base(variant):
    import torch
    from nnfme.runtime import pack_jobs
    jobs, keys = _keyed_jobs()
    depth = _depth(variant)
    if depth == 10:
        keys = (keys * 4).astype(np.int16)      # keys of 10-bit samples (2 * org - pred)
    pk, kb = pack_jobs(jobs)
    assert kb[0] == -1 and kb[1] == 0 and np.all(kb[2:] > 0)
    ctx = _make_ctx(variant, 1)
    orc = _make_oracle(depth, 1)
    ctx.set_keys(keys)                          # the last keyed block ends exactly at n_keys
    orc.set_keys(keys)
    full_p, mv_p, full_u, mv_u, uj = _run4(ctx, jobs)
    assert np.array_equal(uj["key_offset"], jobs["key_offset"])
    _check4(full_p, mv_p, full_u, mv_u, orc.refine(uj), f"keyed {variant}")
    # one sample beyond the key buffer: rejected on the device
    ctx.set_keys(keys[:-1])
    n = len(jobs)
    dpk, dkb = _dev(pk), _dev(kb)
    dr = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.refine_packed_device(dpk.data_ptr(), dkb.data_ptr(), dr.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert ctx.refine_status() > 0
    assert np.all(dr.cpu().numpy().view(RESULT_DTYPE)["status"] == RES_REJECTED)


# ---- test 3: the counters are zero at every batch's start ------------------------------------------
def test_counters_zero_across_rejection_integer_search_and_regrow():
    import torch
    from nnfme.runtime import pack_jobs
    ctx = _make_ctx("d8", 1)                    # max_jobs 0: the work buffers grow with the batches
    orc = _make_oracle(8, 1)
    s = torch.cuda.current_stream()

    def packed(jobs):
        pk, kb = pack_jobs(jobs)
        dpk, dkb = _dev(pk), _dev(kb)
        dr = torch.zeros(len(jobs) * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        ctx.refine_packed_device(dpk.data_ptr(), dkb.data_ptr(), dr.data_ptr(), len(jobs), s.cuda_stream)
        status = ctx.refine_status()
        return dr.cpu().numpy().view(RESULT_DTYPE), status

    def valid(n, seed, what):
        from nnfme.runtime import unpack_jobs
        jobs = _jobs(n, seed)
        got, status = packed(jobs)
        assert status == 0, what
        bad, first, counts = compare_results(got, orc.refine(unpack_jobs(*pack_jobs(jobs))))
        assert bad == 0, f"{what}: {bad} jobs differ from the oracle, first {first}: {counts}"

    valid(700, 31, "first batch")
    before = ctx.nn_get_state()
    bad_jobs = _jobs(700, 32)
    bad_jobs["ref_id"][333] = 40                # an unset picture slot
    got, status = packed(bad_jobs)
    assert status == 1
    assert np.all(got["status"] == RES_REJECTED)
    assert np.array_equal(ctx.nn_get_state(), before)
    valid(650, 33, "after a rejected batch")
    # an integer search on the same context, between two batches
    tz_jobs, ext = synth.make_tz_jobs(np.random.default_rng(34), W, H, 3, 4, [0, 1, 2, 3], [0, 1, 2, 3], search_range=8)
    dj, de = _dev(tz_jobs), _dev(ext)
    ds = torch.zeros(len(tz_jobs), dtype=torch.int32, device="cuda")
    ctx.integer_search_device(dj.data_ptr(), de.data_ptr(), ds.data_ptr(), len(tz_jobs), s.cuda_stream)
    s.synchronize()
    got_tz = dj.cpu().numpy().view(JOB_DTYPE)
    exp_tz, exp_sad = orc.integer_search(tz_jobs, ext)
    assert np.array_equal(got_tz["mv_x"], exp_tz["mv_x"]) and np.array_equal(got_tz["mv_y"], exp_tz["mv_y"])
    assert np.array_equal(ds.cpu().numpy().view(np.uint32), exp_sad)
    valid(700, 35, "after an integer search")
    valid(2600, 36, "after the work buffers regrew")


# ---- test 4: the generic-net tail ------------------------------------------------------------------
def test_deep_tail_reads_packed_jobs():
    net = weights.case_net("scr3x40")
    ctx = _make_ctx("d8", 2, net=net)           # the exact engine (the default)
    jobs = _jobs(1100, 41)
    full_p, mv_p, full_u, mv_u, uj = _run4(ctx, jobs)
    assert len(set(full_p["nn_class"].tolist())) > 1
    _check4(full_p, mv_p, full_u, mv_u, None, "nn_mode 2")
    want = _make_oracle(8, 2, net=net).refine(uj)
    bad, first, counts = compare_results(full_p, want)
    assert bad == 0, f"nn_mode 2: {bad} jobs differ from the oracle, first {first}: {counts}"
