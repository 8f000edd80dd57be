"""The hand-over between overlapped batches on three streams (csrc/fme_overlap_host.h): the front end
of batch k waits for search k - 2, not for batch k - 2, so it may run while the tails of batches k - 2
and k - 3 are pending; what those tails read (blk_prefix, the Schedule, koff, the picture / lambda
tables, which k_front itself writes from its kernel argument) sits in a ring of four entries.

Every check is against the same batches on one stream with a host synchronisation after each, in a
fresh context, byte for byte; the first and last batch of the plain sequence also against the CPU
oracle.  416x240 pictures, 3,024 - 4,928 jobs per batch (synth.make_ctu_jobs): three to five
k_front workgroups and scan blocks.  Ten batches: the ring and the counter blocks round twice, the
three streams three times.  Every batch has its own jobs and lambdas and rebinds one picture, so a
batch that read another batch's tables, schedule or scan carry would give other results."""
import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import JOB_DTYPE, JOB_EMI, MV_FIELDS, MV_RESULT_DTYPE, RES_REJECTED

W, H, QP = 416, 240, 22
NB = 10
LEAD = 8          # leading jobs of batches >= 2 that push fewer than 8 EMI values (they read the carried state)
CALLS = (30, 41, 27, 36, 44, 33, 29, 39, 35, 31)   # per CTU and reference: 28 CTUs x 4 references


def _lambdas(b):
    return [lam * (1.0 + 0.05 * b) for lam in synth.LDP_LAMBDA[QP]]


def _jobs(b, calls=None, seed=None):
    jobs = synth.make_ctu_jobs(np.random.default_rng(700 + b if seed is None else seed), W, H, calls or CALLS[b], 4,
                               [0, 1, 2, 3], [0, 1, 2, 3])
    if b >= 2:
        for i in range(LEAD):
            if i % 2 == 0:
                jobs["flags"][i] &= ~np.uint8(JOB_EMI)
            else:
                jobs["lt_x"][i] = jobs["rb_x"][i] = jobs["mv_x"][i]
    return jobs


_CACHE = {}


def _batches():
    """Batch b binds picture b % 5 anew (pictures 0 - 3: references, 4: the original); batch 0 binds all five."""
    if "batches" not in _CACHE:
        out = []
        for b in range(NB):
            pics = {i: synth.synth_luma(W, H, i) for i in range(5)} if b == 0 else {b % 5: synth.synth_luma(W, H, 20 + b)}
            out.append({"pics": pics, "lam": _lambdas(b), "jobs": _jobs(b)})
        _CACHE["batches"] = out
    return _CACHE["batches"]


def _oracle_first_and_last():
    """The oracle's records of batches 0 and NB - 1, the NN state carried through all of them."""
    if "oracle" not in _CACHE:
        from oracle import Oracle
        o = Oracle(use_hadamard=1, nn_mode=1, qp=QP, fast_inter_mode=1)
        o.load_nn(weights.load_weights(QP))
        out = {}
        for b, bt in enumerate(_batches()):
            for k, v in bt["pics"].items():
                o.set_picture(k, v)
            for lid, lam in enumerate(bt["lam"]):
                o.set_lambda(lid, lam)
            r = o.refine(bt["jobs"])
            if b in (0, NB - 1):
                out[b] = r
        _CACHE["oracle"] = out
    return _CACHE["oracle"]


def _ctx():
    from nnfme.runtime import FmeContext
    return FmeContext(device=0, use_hadamard=1, nn_mode=1, qp=QP, fast_inter_mode=1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _run(batches, n_streams, sync_each=False, keys=None, tz=None, extra=None):
    """The batches in order on a fresh context, batch b on stream b % n_streams (stream 0: the current
    stream).  sync_each: the host waits for the device after every batch (the serial reference) and
    records each batch's rejected-job count; otherwise nothing waits between the batches.  A batch
    with "packed" is issued as fme_job_packed rows.  keys: {b: (requests, key count)} device-built
    keys enqueued before batch b on its stream; tz: {b: (jobs, ext)} an integer search before batch b
    on its stream.  Returns the batches' fme_mv_result rows and the last NN state; extra receives
    "rejected" (per batch with sync_each, else the last batch's) and "tz"."""
    import torch
    from nnfme.runtime import pack_jobs
    ctx = _ctx()
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]
    d_pics = [{k: _dev(v) for k, v in bt["pics"].items()} for bt in batches]
    d_jobs = []
    for bt in batches:
        if bt.get("packed"):
            pk, kb = pack_jobs(bt["jobs"])
            d_jobs.append((_dev(pk), _dev(kb)))
        else:
            d_jobs.append((_dev(bt["jobs"]), None))
    d_reqs = {b: _dev(r) for b, (r, _) in (keys or {}).items()}
    d_out = [torch.zeros(len(bt["jobs"]) * MV_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for bt in batches]
    d_tz = {b: (_dev(j), _dev(e), torch.zeros(len(j), dtype=torch.int32, device="cuda")) for b, (j, e) in (tz or {}).items()}
    torch.cuda.synchronize()   # the inputs are in place before any stream reads them
    rejected = []
    for b, bt in enumerate(batches):
        s = streams[b % n_streams].cuda_stream
        for k, t in d_pics[b].items():
            ctx.bind_picture_device(k, t.data_ptr(), W, W, H)
        for lid, lam in enumerate(bt["lam"]):
            ctx.set_lambda(lid, lam)
        if keys and b in keys:
            ctx.build_bipred_keys_device(d_reqs[b].data_ptr(), len(keys[b][0]), keys[b][1], s)
        if tz and b in tz:
            ctx.integer_search_device(d_tz[b][0].data_ptr(), d_tz[b][1].data_ptr(), d_tz[b][2].data_ptr(), len(tz[b][0]), s)
        n = len(bt["jobs"])
        if d_jobs[b][1] is not None:
            ctx.refine_mv_packed_device(d_jobs[b][0].data_ptr(), d_jobs[b][1].data_ptr(), d_out[b].data_ptr(), n, s)
        else:
            ctx.refine_mv_device(d_jobs[b][0].data_ptr(), d_out[b].data_ptr(), n, s)
        if sync_each:
            rejected.append(ctx.refine_status())
            torch.cuda.synchronize()
    if not sync_each:
        rejected.append(ctx.refine_status())   # of the batch issued last (waits for it)
    for s in streams:
        s.synchronize()
    out = [t.cpu().numpy().view(MV_RESULT_DTYPE).copy() for t in d_out]
    state = ctx.nn_get_state()
    if extra is not None:
        extra["rejected"] = rejected
        extra["tz"] = {}
        for b, (dj, _, ds) in d_tz.items():
            j = dj.cpu().numpy().view(JOB_DTYPE)
            extra["tz"][b] = (j["mv_x"].copy(), j["mv_y"].copy(), ds.cpu().numpy().copy())
    ctx.close()
    return out, state


def _assert_equal_runs(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (
            f"{what}: batch {b}: " + ", ".join(f"{f} {int(np.sum(g[f] != w[f]))}" for f in MV_RESULT_DTYPE.names) +
            f" of {len(g)} rows differ")


def _serial():
    if "serial" not in _CACHE:
        _CACHE["serial"] = _run(_batches(), 1, sync_each=True)
    return _CACHE["serial"]


@pytest.mark.gpu
def test_rotation_on_three_streams_equals_serial_and_the_oracle():
    want, want_state = _serial()
    got, got_state = _run(_batches(), 3)
    _assert_equal_runs(got, want, "three streams against one with a wait after each batch")
    assert np.array_equal(got_state, want_state)
    assert not any(np.any(g["status"] & RES_REJECTED) for g in got)
    orc = _oracle_first_and_last()
    for b in (0, NB - 1):
        for f in MV_FIELDS:
            assert np.array_equal(got[b][f], orc[b][f]), f"batch {b} field {f} against the oracle"


def _featured():
    """The plain batches with, in the middle: device-built keys before batch 1 and a packed batch with
    keyed jobs as batch 3 (not serialised: batches 4 and 5 have their front ends while its tail, which
    reads koff, may be pending); an integer search before batch 6; two invalid jobs in batch 8."""
    if "featured" not in _CACHE:
        batches = [dict(bt) for bt in _batches()]
        jobs = synth.make_ctu_jobs(np.random.default_rng(77), W, H, 32, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=0.3)
        reqs, kc = synth.make_bipred_key_reqs(np.random.default_rng(78), jobs, 4, [0, 1, 2, 3])
        batches[3]["jobs"] = jobs
        batches[3]["packed"] = True
        batches[5]["packed"] = True   # and a packed batch without keyed jobs
        bad = batches[8]["jobs"].copy()
        bad["w"][len(bad) // 2] = 20          # no such PU shape
        bad["ref_id"][len(bad) - 3] = 9       # an unset picture slot
        batches[8]["jobs"] = bad
        tzj, tze = synth.make_tz_jobs(np.random.default_rng(906), W, H, 12, 4, [0, 1, 2, 3], [0, 1, 2, 3])
        _CACHE["featured"] = (batches, {1: (reqs, kc)}, {6: (tzj, tze)})
    return _CACHE["featured"]


@pytest.mark.gpu
def test_rotation_with_keyed_batch_integer_search_and_rejected_batch():
    batches, keys, tz = _featured()
    xs, x3 = {}, {}
    want, want_state = _run(batches, 1, sync_each=True, keys=keys, tz=tz, extra=xs)
    got, got_state = _run(batches, 3, keys=keys, tz=tz, extra=x3)
    _assert_equal_runs(got, want, "keyed batch 3, integer search before batch 6, batch 8 rejected")
    assert np.array_equal(got_state, want_state)
    assert xs["rejected"] == [0] * 8 + [2, 0]          # batch 8 alone, and both of its jobs
    assert x3["rejected"] == [0]                        # the last batch saw its own Schedule
    assert np.all(got[8]["status"] == RES_REJECTED)
    for b in range(NB):
        if b != 8:
            assert not np.any(got[b]["status"] & RES_REJECTED), f"batch {b}"
    assert np.any(batches[3]["jobs"]["key_offset"] >= 0)
    for a, w, f in zip(x3["tz"][6], xs["tz"][6], ("mv_x", "mv_y", "sad")):
        assert np.array_equal(a, w), f"integer search before batch 6: {f}"
    assert np.any(x3["tz"][6][2] != 0)
    # the batches before the first feature are the plain sequence's
    _assert_equal_runs(got[:1], _serial()[0][:1], "before the keys")
    # the rejected batch issued last, its predecessors valid: the count read back is its own
    x4 = {}
    first = dict(batches[5], pics={i: synth.synth_luma(W, H, i) for i in range(5)})
    _run([first] + batches[6:9], 3, extra=x4)
    assert x4["rejected"] == [2]


@pytest.mark.gpu
def test_short_batches_while_a_long_tail_is_pending():
    """40,096 jobs on one stream, then 64 and 3,024 jobs at once on the other two: the short batches'
    front ends run while the long batch's tail is pending."""
    base = _batches()
    batches = [
        {"pics": base[0]["pics"], "lam": _lambdas(0), "jobs": _jobs(2, calls=358, seed=811)},
        {"pics": base[1]["pics"], "lam": _lambdas(1), "jobs": _jobs(2, seed=812)[:64].copy()},
        {"pics": base[2]["pics"], "lam": _lambdas(2), "jobs": _jobs(2, calls=27, seed=813)},
    ]
    assert [len(bt["jobs"]) for bt in batches] == [40096, 64, 3024]
    want, want_state = _run(batches, 1, sync_each=True)
    got, got_state = _run(batches, 3)
    _assert_equal_runs(got, want, "long batch, then two short ones")
    assert np.array_equal(got_state, want_state)
    assert not any(np.any(g["status"] & RES_REJECTED) for g in got)


@pytest.mark.gpu
def test_frame_replay_one_two_and_three_compute_streams():
    import torch
    from nnfme.pipeline import FrameReplay
    base = synth.make_ctu_jobs(np.random.default_rng(43), W, H, 30, 4, [0, 1, 2, 3], [0])
    pool = np.stack([synth.synth_luma(W, H, t) for t in range(8)])
    lam = lambda f: synth.LDP_LAMBDA[QP][(f + 1) % 4]   # noqa: E731
    steps = 6
    rows = {}
    for cs in (1, 2, 3):
        ctx = _ctx()
        rep = FrameReplay(ctx, base, pool, lam, steps, device=torch.device("cuda", 0), compute_streams=cs)
        assert len(rep.s_comps) == cs
        rep.prime()
        for k in range(steps):
            rep.issue(k)
        rep.finish()
        rep.check_status()
        rows[cs] = [rep.results(k).copy() for k in range(steps)]
        rep.close()
        ctx.close()
    for k in range(steps):
        assert rows[2][k].tobytes() == rows[1][k].tobytes(), f"two streams, step {k}"
        assert rows[3][k].tobytes() == rows[1][k].tobytes(), f"three streams, step {k}"
    assert len({r.tobytes() for r in rows[1]}) == steps


def test_default_replay_rotates_three_streams():
    """On the CPU: the replay's default and the stream counts it accepts."""
    import inspect
    from nnfme.pipeline import FrameReplay
    assert inspect.signature(FrameReplay.__init__).parameters["compute_streams"].default == 3
