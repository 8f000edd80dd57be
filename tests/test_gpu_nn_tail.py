"""The NN tail kernel (k_nn_tail) at its seams: wave, round and scan-block boundaries, jobs that
read their NN inputs from an earlier job of the batch or from the state carried in from the batch
before, and jobs at a search-range edge that push fewer than 8 distortions.

Batches of mixed PU shapes on a 256x256 picture set, with the QP 22 and the QP 37 nets, through
both job forms (fme_job and packed rows).  Every field of fme_mv_result and the carried NN state
must equal the CPU oracle's on the same jobs, after the batch and after a second batch chained on
it: exact equality, no tolerance.  A last batch puts the writers many waves back: long stretches
of jobs that push nothing, one over a whole scan block, and edge jobs that push some slots only."""
import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import JOB_EMI, MV_FIELDS, MV_RESULT_DTYPE

pytestmark = pytest.mark.gpu

W, H = 256, 256
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)   # one wave, one 1024-job scan block, each +-1; a third block of one job
QPS = (22, 37)
N_SECOND = 130                                     # the chained batch: two waves and a part of a third

_PICS = {}


def _bind(eng, qp):
    if not _PICS:
        _PICS.update({i: synth.synth_luma(W, H, i) for i in range(5)})
    for k, v in _PICS.items():
        eng.set_picture(k, v)
    for lid, lam in enumerate(synth.LDP_LAMBDA[qp]):
        eng.set_lambda(lid, lam)


def _jobs(n, seed, no_emi_phase):
    """n canonical jobs (what the device unpacks from packed rows) and their packed form.  The first
    24 are the 24 PU shapes, the next 16 sit at the search-range edge with every combination of the
    four range bits, and every third job (i % 3 == no_emi_phase) carries no FME_JOB_EMI: it pushes
    nothing and reads the state the jobs before it left."""
    from nnfme.runtime import pack_jobs, unpack_jobs
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
    jobs["flags"][no_emi_phase::3] &= ~np.uint8(JOB_EMI)
    pk, kb = pack_jobs(jobs)
    return unpack_jobs(pk, kb), pk, kb


def _batches(n):
    """The batch of n jobs and the batch chained on it; job 0 of the second has no EMI, so it takes
    every NN input from the state the first batch carried over."""
    return _jobs(n, 300 + n, 2), _jobs(N_SECOND, 900 + n, 0)


_CTX, _ORC, _WANT = {}, {}, {}


def _ctx(qp):
    if qp not in _CTX:
        from nnfme.runtime import FmeContext
        _CTX[qp] = FmeContext(nn_mode=1, qp=qp)
        _bind(_CTX[qp], qp)
    return _CTX[qp]


def _oracle(qp, n):
    """[(results, state after)] of the two chained batches from a reset state, once per (qp, n)."""
    if (qp, n) not in _WANT:
        if qp not in _ORC:
            from oracle import Oracle
            _ORC[qp] = Oracle(nn_mode=1, qp=qp)
            _bind(_ORC[qp], qp)
            _ORC[qp].load_nn(weights.load_weights(qp))
        o = _ORC[qp]
        o.nn_reset()
        out = []
        for uj, _, _ in _batches(n):
            res = o.refine(uj)
            out.append((res, o.nn_get_state()))
        _WANT[qp, n] = out
    return _WANT[qp, n]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _run(ctx, form, batch):
    import torch
    uj, pk, kb = batch
    n = len(uj)
    s = torch.cuda.current_stream().cuda_stream
    d = torch.zeros(n * MV_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    if form == "packed":
        dpk, dkb = _dev(pk), _dev(kb)
        ctx.refine_mv_packed_device(dpk.data_ptr(), dkb.data_ptr(), d.data_ptr(), n, s)
    else:
        duj = _dev(uj)
        ctx.refine_mv_device(duj.data_ptr(), d.data_ptr(), n, s)
    assert ctx.refine_status() == 0
    return d.cpu().numpy().view(MV_RESULT_DTYPE)


@pytest.mark.parametrize("form", ["fme_job", "packed"])
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("n", SIZES)
def test_tail_equals_oracle_across_seams(n, qp, form):
    batches = _batches(n)
    want = _oracle(qp, n)
    first = want[0][0]
    assert len(MV_FIELDS) == len(MV_RESULT_DTYPE.names) - 1          # every field but the reserved byte
    if n >= 64:
        assert len(set(zip(batches[0][0]["w"].tolist(), batches[0][0]["h"].tolist()))) == 24
        emi = (batches[0][0]["flags"] & JOB_EMI) != 0
        assert not emi[2::3].any() and emi[0::3].all() and emi[1::3].all()
        edge = first["n_emi"][24:40][emi[24:40]]
        assert (edge < 8).sum() >= 8 and len(set(edge.tolist())) > 3, "edge jobs that push fewer than 8 distortions"
        assert (first["n_emi"][~emi] == 0).all()
    ctx = _ctx(qp)
    ctx.nn_reset()
    for k, (batch, (res, state)) in enumerate(zip(batches, want)):
        got = _run(ctx, form, batch)
        what = f"n={n} qp={qp} {form} batch {k}"
        for f in MV_FIELDS:
            bad = np.flatnonzero(got[f] != res[f])
            assert bad.size == 0, f"{what}: fme_mv_result.{f} differs from the oracle at {bad[:8].tolist()} ({bad.size} jobs)"
        assert np.array_equal(ctx.nn_get_state(), state), f"{what}: NN state differs from the oracle"
    assert len(set(first["nn_class"].tolist())) > 1 or n < 63


def _stretch_jobs():
    """2,300 jobs whose last writers lie far back: jobs 100..399 and 1000..2099 carry no
    FME_JOB_EMI (whole waves without a writer, the second stretch across a scan-block start and
    over the whole scan block 1024..2047, whose carry-in is then a job of the block before), and
    jobs 600..799 sit at a search-range edge with every combination of the range bits, so the
    slots they do not push were written up to three waves earlier, each slot at its own distance."""
    from nnfme.runtime import pack_jobs, unpack_jobs
    n = 2300
    rng = np.random.default_rng(77)
    jobs = synth.make_jobs(rng, W, H, n, 4, [0, 1, 2, 3], [0, 1, 2, 3])
    for i in range(600, 800):
        b = int(rng.integers(0, 16))
        jobs["lt_x"][i] = jobs["mv_x"][i] - (b & 1)
        jobs["rb_x"][i] = jobs["mv_x"][i] + ((b >> 1) & 1)
        jobs["lt_y"][i] = jobs["mv_y"][i] - ((b >> 2) & 1)
        jobs["rb_y"][i] = jobs["mv_y"][i] + ((b >> 3) & 1)
    jobs["flags"][100:400] &= ~np.uint8(JOB_EMI)
    jobs["flags"][1000:2100] &= ~np.uint8(JOB_EMI)
    pk, kb = pack_jobs(jobs)
    return unpack_jobs(pk, kb), pk, kb


@pytest.mark.parametrize("form", ["fme_job", "packed"])
def test_tail_writers_many_waves_back(form):
    batch = _stretch_jobs()
    if "stretch" not in _WANT:
        _oracle(22, 1)                       # binds the QP 22 oracle
        o = _ORC[22]
        o.nn_reset()
        _WANT["stretch"] = (o.refine(batch[0]), o.nn_get_state())
    res, state = _WANT["stretch"]
    assert (res["n_emi"][100:400] == 0).all() and (res["n_emi"][1000:2100] == 0).all()
    assert len(set(res["n_emi"][600:800].tolist())) > 4 and (res["n_emi"][600:800] < 8).sum() > 150
    ctx = _ctx(22)
    ctx.nn_reset()
    got = _run(ctx, form, batch)
    for f in MV_FIELDS:
        bad = np.flatnonzero(got[f] != res[f])
        assert bad.size == 0, f"{form}: fme_mv_result.{f} differs from the oracle at {bad[:8].tolist()} ({bad.size} jobs)"
    assert np.array_equal(ctx.nn_get_state(), state), f"{form}: NN state differs from the oracle"


def test_the_two_nets_disagree():
    """The QP 22 and QP 37 weights give different classes on the same jobs, so neither case stands
    in for the other."""
    a, b = _oracle(22, 1025)[0][0], _oracle(37, 1025)[0][0]
    assert (a["nn_class"] != b["nn_class"]).any()
