"""Consecutive refinement batches on two streams (csrc/fme_overlap_host.h): batch k+1's front end and
search run on another stream than batch k's and do not wait for batch k's tail.  Every check is
against the same sequence on one stream in a fresh context (computed once per sequence and shared),
and one batch against the CPU oracle.

416x240 pictures, 1,568 - 2,912 jobs per batch (synth.make_ctu_jobs): more than one 1,024-job scan
block and several wave tiles per class.  Nine batches: both slots, and the four counter blocks
round twice.  Every batch has its own pictures, lambdas and jobs, so a batch that read another
batch's tables, class order or schedule would give other results."""
import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import JOB_DTYPE, JOB_EMI, MV_FIELDS, MV_RESULT_DTYPE, RES_REJECTED

W, H, QP = 416, 240, 22
NB = 9
LEAD = 8          # leading jobs of batches >= 2 that push fewer than 8 EMI values
CALLS = (14, 26, 17, 23, 15, 25, 19, 21, 16)   # per CTU and reference: 28 CTUs x 4 references
# job seeds, chosen so that the carried state changes at least three of the leading classes of every
# batch from the third on (test_leading_jobs_depend_on_the_carried_state asserts it on the CPU)
SEEDS = (500, 501, 502, 603, 504, 1205, 506, 507, 508)


def _lambdas(b):
    return [lam * (1.0 + 0.06 * b) for lam in synth.LDP_LAMBDA[QP]]


def _pictures(b):
    return {i: synth.synth_luma(W, H, 10 * b + i) for i in range(5)}


def _jobs(b):
    jobs = synth.make_ctu_jobs(np.random.default_rng(SEEDS[b]), W, H, CALLS[b], 4, [0, 1, 2, 3], [0, 1, 2, 3])
    if b >= 2:
        # the first LEAD jobs read the previous batch's carried NN state: every other one without
        # FME_JOB_EMI (no push at all), the rest range-limited to their start (fewer than 8 pushes)
        for i in range(LEAD):
            if i % 2 == 0:
                jobs["flags"][i] &= ~np.uint8(JOB_EMI)
            else:
                jobs["lt_x"][i] = jobs["rb_x"][i] = jobs["mv_x"][i]
    return jobs


_CACHE = {}


def _batches():
    if "batches" not in _CACHE:
        _CACHE["batches"] = [{"pics": _pictures(b), "lam": _lambdas(b), "jobs": _jobs(b)} for b in range(NB)]
    return _CACHE["batches"]


def _oracle():
    from oracle import Oracle
    o = Oracle(use_hadamard=1, nn_mode=1, qp=QP, fast_inter_mode=1)
    o.load_nn(weights.load_weights(QP))
    return o


def _oracle_bind(o, bt):
    for k, v in bt["pics"].items():
        o.set_picture(k, v)
    for lid, lam in enumerate(bt["lam"]):
        o.set_lambda(lid, lam)


def _oracle_sequence():
    """The oracle's records of every batch, the NN state carried from batch to batch."""
    if "oracle" not in _CACHE:
        o = _oracle()
        out = []
        for bt in _batches():
            _oracle_bind(o, bt)
            out.append(o.refine(bt["jobs"]))
        _CACHE["oracle"] = out
    return _CACHE["oracle"]


def _ctx():
    from nnfme.runtime import FmeContext
    return FmeContext(device=0, use_hadamard=1, nn_mode=1, qp=QP, fast_inter_mode=1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _run(batches, n_streams, before=None, keys=None, tz=None, reset_and_copy=False, extra=None):
    """The batches in order on a fresh context, batch b on stream b % n_streams (stream 0: the
    current stream), with no host synchronisation between them.  before: {b: f(ctx)} host calls
    made right before batch b is enqueued; keys: {b: (requests, key count)} device-built keys of
    batch b; tz: {b: (jobs, ext, other)} an integer search on batch b's pictures enqueued before
    batch b, on batch b's stream or (other) on the stream batch b does not use; reset_and_copy:
    every batch starts from a reset NN state and its end state is copied on the device right after
    it (what a sharded replay does per step).  Returns the batches' fme_mv_result rows and the last
    NN state; extra (a dict) receives "tz" {b: (mv_x, mv_y, sad)} and "states" [NB][12]."""
    import torch
    ctx = _ctx()
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]
    d_pics = [{k: _dev(v) for k, v in bt["pics"].items()} for bt in batches]
    d_jobs = [_dev(bt["jobs"]) for bt in batches]
    d_reqs = {b: _dev(r) for b, (r, _) in (keys or {}).items()}
    d_out = [torch.zeros(len(bt["jobs"]) * MV_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for bt in batches]
    d_tz = {b: (_dev(j), _dev(e), torch.zeros(len(j), dtype=torch.int32, device="cuda")) for b, (j, e, _) in (tz or {}).items()}
    d_states = torch.zeros((len(batches), 12), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # the inputs are in place before any stream reads them
    for b, bt in enumerate(batches):
        s = streams[b % n_streams].cuda_stream
        for k, t in d_pics[b].items():
            ctx.bind_picture_device(k, t.data_ptr(), W, W, H)
        for lid, lam in enumerate(bt["lam"]):
            ctx.set_lambda(lid, lam)
        if before and b in before:
            before[b](ctx)
        if keys and b in keys:
            ctx.build_bipred_keys_device(d_reqs[b].data_ptr(), len(keys[b][0]), keys[b][1], s)
        if tz and b in tz:
            zs = streams[(b + 1) % n_streams].cuda_stream if tz[b][2] else s
            ctx.integer_search_device(d_tz[b][0].data_ptr(), d_tz[b][1].data_ptr(), d_tz[b][2].data_ptr(), len(tz[b][0]), zs)
        if reset_and_copy:
            ctx.nn_reset()
        ctx.refine_mv_device(d_jobs[b].data_ptr(), d_out[b].data_ptr(), len(bt["jobs"]), s)
        if reset_and_copy:
            ctx.nn_copy_state_device(d_states[b].data_ptr(), s)
    for s in streams:
        s.synchronize()
    out = [t.cpu().numpy().view(MV_RESULT_DTYPE).copy() for t in d_out]
    state = ctx.nn_get_state()
    if extra is not None:
        extra["states"] = d_states.cpu().numpy().view(np.uint32).copy()
        extra["tz"] = {}
        for b, (dj, _, ds) in d_tz.items():
            j = dj.cpu().numpy().view(JOB_DTYPE)
            extra["tz"][b] = (j["mv_x"].copy(), j["mv_y"].copy(), ds.cpu().numpy().copy())
    ctx.close()
    return out, state


def _assert_equal_runs(got, want, what, skip=()):
    for b, (g, w) in enumerate(zip(got, want)):
        if b in skip:
            continue
        for f in sorted(set(MV_FIELDS) | {"status"}):
            bad = np.flatnonzero(g[f] != w[f])
            assert bad.size == 0, f"{what}: batch {b} field {f}: {bad.size} of {len(g)} rows differ (first {bad[:5]})"


def _serial():
    if "serial" not in _CACHE:
        _CACHE["serial"] = _run(_batches(), 1)
    return _CACHE["serial"]


def test_leading_jobs_depend_on_the_carried_state():
    """On the CPU: the oracle's classes of the leading jobs of every batch from the third on differ
    when the carry-in is zeroed, so a tail that ran before the previous batch's tail would show."""
    want = _oracle_sequence()
    o = _oracle()
    for b in range(2, NB):
        bt = _batches()[b]
        _oracle_bind(o, bt)
        o.nn_reset()
        fresh = o.refine(bt["jobs"][:LEAD])
        differ = int(np.sum(fresh["nn_class"] != want[b]["nn_class"][:LEAD]))
        assert differ >= 3, f"batch {b}: the carried state changes {differ} leading classes"


@pytest.mark.gpu
def test_two_streams_equal_one_stream_and_the_oracle():
    want, want_state = _serial()
    got, got_state = _run(_batches(), 2)
    _assert_equal_runs(got, want, "two streams against one")
    assert np.array_equal(got_state, want_state)
    orc = _oracle_sequence()
    for b in (0, 5):   # a first batch and one in steady state, against the CPU oracle
        for f in MV_FIELDS:
            assert np.array_equal(got[b][f], orc[b][f]), f"batch {b} field {f} against the oracle"
    # the carried state crossed the streams: the leading jobs' classes are the oracle's
    for b in range(2, NB):
        assert np.array_equal(got[b]["nn_class"][:LEAD], orc[b]["nn_class"][:LEAD]), f"batch {b}: leading classes"


@pytest.mark.gpu
def test_rejected_batch_in_the_middle():
    batches = [dict(bt) for bt in _batches()]
    bad = batches[3]["jobs"].copy()
    bad["w"][len(bad) // 2] = 20   # no such PU shape: the device rejects the whole batch
    batches[3]["jobs"] = bad
    want, want_state = _run(batches, 1)
    got, got_state = _run(batches, 2)
    assert np.all(got[3]["status"] == RES_REJECTED) and np.all(want[3]["status"] == RES_REJECTED)
    _assert_equal_runs(got, want, "with batch 3 rejected", skip=(3,))
    assert np.array_equal(got_state, want_state)
    # and the batches before it are what they are without the rejection
    _assert_equal_runs(got[:3], _serial()[0][:3], "before the rejected batch")


@pytest.mark.gpu
def test_keyed_batch_between_uni_pred_batches():
    batches = [dict(bt) for bt in _batches()[:5]]
    jobs = synth.make_ctu_jobs(np.random.default_rng(77), W, H, 18, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=0.3)
    reqs, kc = synth.make_bipred_key_reqs(np.random.default_rng(78), jobs, 4, [0, 1, 2, 3])
    batches[2]["jobs"] = jobs
    keys = {2: (reqs, kc)}
    want, _ = _run(batches, 1, keys=keys)
    got, _ = _run(batches, 2, keys=keys)
    assert not np.any(got[2]["status"] & RES_REJECTED)
    _assert_equal_runs(got, want, "keyed batch in the middle")


@pytest.mark.gpu
def test_state_set_and_reset_between_overlapped_batches():
    st = np.array([3, 1, 4, 1, 5, 9, 2, 6, 40, 16, 8, 1], np.uint32)
    before = {4: lambda ctx: ctx.nn_set_state(st), 6: lambda ctx: ctx.nn_reset()}
    want, want_state = _run(_batches(), 1, before=before)
    got, got_state = _run(_batches(), 2, before=before)
    _assert_equal_runs(got, want, "state set before batch 4, reset before batch 6")
    assert np.array_equal(got_state, want_state)
    plain = _serial()[0]
    _assert_equal_runs(got[:4], plain[:4], "before the set")
    for b in (4, 6):   # the set / reset reached the batch's leading jobs
        assert np.any(got[b]["nn_class"][:LEAD] != plain[b]["nn_class"][:LEAD]), f"batch {b}: state change without effect"


@pytest.mark.gpu
def test_frame_replay_two_compute_streams_equal_one():
    import torch
    from nnfme.pipeline import FrameReplay
    base = synth.make_ctu_jobs(np.random.default_rng(43), W, H, 20, 4, [0, 1, 2, 3], [0])
    pool = np.stack([synth.synth_luma(W, H, t) for t in range(8)])
    lam = lambda f: synth.LDP_LAMBDA[QP][(f + 1) % 4]   # noqa: E731
    rows = {}
    for cs in (1, 2):
        ctx = _ctx()
        rep = FrameReplay(ctx, base, pool, lam, 4, device=torch.device("cuda", 0), compute_streams=cs)
        rep.prime()
        for k in range(4):
            rep.issue(k)
        rep.finish()
        rep.check_status()
        rows[cs] = [rep.results(k).copy() for k in range(4)]
        rep.close()
        ctx.close()
    for k in range(4):
        assert np.array_equal(rows[2][k], rows[1][k]), f"step {k}"


@pytest.mark.gpu
def test_integer_search_between_overlapped_batches():
    """An integer search before batch 2 on the stream batch 2 does not use, and one before batch 5 on
    batch 5's own stream: it takes a batch number, a slot and a counter block like a batch, and the
    batches around it, on either stream, neither zero its counters nor have theirs zeroed."""
    tz = {}
    for b, other in ((2, True), (5, False)):
        jobs, ext = synth.make_tz_jobs(np.random.default_rng(900 + b), W, H, 12, 4, [0, 1, 2, 3], [0, 1, 2, 3])
        tz[b] = (jobs, ext, other)
    xs, x2 = {}, {}
    want, want_state = _run(_batches(), 1, tz=tz, extra=xs)
    got, got_state = _run(_batches(), 2, tz=tz, extra=x2)
    _assert_equal_runs(got, want, "integer searches before batches 2 and 5")
    assert np.array_equal(got_state, want_state)
    _assert_equal_runs(got, _serial()[0], "against the run without integer searches")
    for b in tz:
        for a, w, f in zip(x2["tz"][b], xs["tz"][b], ("mv_x", "mv_y", "sad")):
            assert np.array_equal(a, w), f"integer search before batch {b}: {f}"
        assert np.any(x2["tz"][b][2] != 0)


@pytest.mark.gpu
def test_reset_batch_and_state_copy_per_step():
    """What a sharded replay does per step, on alternating streams: reset, batch, device copy of the
    end state.  Batch k+1's reset writes the words batch k's copy reads, on the other stream: every
    copied state must be that batch's end state, as on one stream."""
    xs, x2 = {}, {}
    want, _ = _run(_batches(), 1, reset_and_copy=True, extra=xs)
    got, _ = _run(_batches(), 2, reset_and_copy=True, extra=x2)
    _assert_equal_runs(got, want, "reset + batch + state copy per step")
    assert np.array_equal(x2["states"], xs["states"])
    # real end states (word 11: the fields written so far; a reset state is all zero), all distinct
    assert np.all(xs["states"][:, 11] != 0) and len({tuple(r) for r in xs["states"]}) == NB
