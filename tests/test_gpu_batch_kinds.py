"""Every kind of batch after every other on one context (csrc/fme_api.cpp, the batch scaffold): an
ordinary batch, an NN-direct batch, an inputs batch, an evaluation batch, an integer search and another
ordinary batch, enqueued on two streams with no host synchronisation in between, against the same
calls made one by one, each on a fresh context primed with fme_nn_set_state from the call before.
The other GPU tests interleave the kinds pairwise; this one pins what the kinds share: the plan and
its waits, the hand-over of the NN state, and the bookkeeping a finished batch leaves.

The fixture's jobs are cut into consecutive pieces of a few dozen jobs; the second spans two tail
waves (70 jobs).  The calls, in order (A, B: two streams):
  1. fme_refine_device             piece 1                                              A
  2. fme_refine_direct_device      piece 2                                              B
  3. fme_nn_inputs_device          piece 3                                              A
  4. fme_refine_at_device          piece 3's jobs (the rows are theirs), the rows step 3
                                   wrote, the classes of the fixture's oracle records   B
  5. fme_integer_search_device     a copy of piece 5 (the search writes its jobs)       A
  6. fme_refine_device             piece 4                                              B
then fme_nn_copy_state_device.  In the second case one job of piece 3 has w = 20: steps 3 and 4 are
rejected whole, the NN state passes through them, and step 6 gives what it gives without piece 3.
Every comparison is == on integers, on every field."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from nnfme import direct, predictor
from nnfme.abi import JOB_DTYPE, RES_REJECTED, RESULT_DTYPE, TZ_EXT_DTYPE
from nnfme.predictor import NN_ROW_DTYPE
from test_gpu_direct import _close, _host, _open, _records, _same, _upload

pytestmark = pytest.mark.gpu

CUTS = (0, 41, 111, 148, 200, 245)   # pieces of 41, 70, 37, 52 and 45 jobs
BAD = 17                             # the job of piece 3 that the second case spoils


def _pieces(name, reject):
    g = load_golden(name)
    jobs = np.ascontiguousarray(g["jobs"])
    p = [jobs[a:b].copy() for a, b in zip(CUTS[:-1], CUTS[1:])]
    if reject:
        p[2]["w"][BAD] = 20
    cls = np.ascontiguousarray(g["results"]["nn_class"][CUTS[2]:CUTS[3]]).astype(np.uint8)
    assert cls.max() < 49 and max(len(q) for q in p) >= 65
    ext = np.zeros(len(p[4]), TZ_EXT_DTYPE)   # the integer search: each PU its own CU, 8 samples of range
    ext["cu_x"], ext["cu_y"], ext["search_range"] = p[4]["x"], p[4]["y"], 8
    return p, cls, ext


def _buffers(p, cls, ext, rows=None):
    """The device buffers of the six steps, complete before anything is enqueued.  rows: step 3's
    output from an earlier run (step 4 alone)."""
    import torch
    d = {1: (_upload(p[0]), _records(len(p[0]))),
         2: (_upload(p[1]), _records(len(p[1]))),
         3: (_upload(p[2]), _records(len(p[2]), NN_ROW_DTYPE) if rows is None else _upload(rows)),
         4: (torch.from_numpy(cls).cuda(), _records(len(p[2]))),
         5: (_upload(p[4]), _upload(ext), torch.zeros(len(p[4]), dtype=torch.int32, device="cuda")),
         6: (_upload(p[3]), _records(len(p[3])))}
    torch.cuda.synchronize()
    return d


def _enqueue(ctx, d, p, steps, a=None, b=None):
    if 1 in steps:
        ctx.refine_device(d[1][0].data_ptr(), d[1][1].data_ptr(), len(p[0]), a)
    if 2 in steps:
        direct.refine_direct_device(ctx, d[2][0], d[2][1], len(p[1]), b)
    if 3 in steps:
        predictor.nn_inputs_device(ctx, d[3][0], d[3][1], len(p[2]), a)
    if 4 in steps:
        predictor.refine_at_device(ctx, d[3][0], d[3][1], d[4][0], d[4][1], len(p[2]), b)
    if 5 in steps:
        ctx.integer_search_device(d[5][0].data_ptr(), d[5][1].data_ptr(), d[5][2].data_ptr(), len(p[4]), a)
    if 6 in steps:
        ctx.refine_device(d[6][0].data_ptr(), d[6][1].data_ptr(), len(p[3]), b)


def _read(d, step):
    """What step `step` wrote, on the host."""
    if step == 3:
        return (_host(d[3][1], NN_ROW_DTYPE),)
    if step == 5:
        return _host(d[5][0], JOB_DTYPE), d[5][2].cpu().numpy().view(np.uint32)
    return (_host(d[step][1]),)


@functools.lru_cache(maxsize=None)
def _one_by_one(name, reject):
    """Per step: what it writes, then the NN state behind it; each step alone on a fresh context that
    starts from the state the step before left (computed once per case, read only)."""
    import torch
    p, cls, ext = _pieces(name, reject)
    out, state, rows = {}, None, None
    for step in range(1, 7):
        _, ctx, _, keep = _open(name)
        try:
            if state is not None:
                ctx.nn_set_state(state)
            d = _buffers(p, cls, ext, rows if step == 4 else None)
            _enqueue(ctx, d, p, {step})
            torch.cuda.synchronize()
            state = ctx.nn_get_state()
            out[step] = _read(d, step) + (state,)
        finally:
            _close(ctx)
        if step == 3:
            rows = out[3][0]
        for arr in out[step]:
            arr.setflags(write=False)
    return out


def _blank(n, dtype):
    out = np.zeros(n, dtype)
    out["status"] = RES_REJECTED
    return out


@pytest.mark.parametrize("reject", [False, True], ids=["valid", "piece3_rejected"])
@pytest.mark.parametrize("name", ["fen3_qp27_nn", "main10_fen3_qp27_nn"])
def test_every_kind_after_every_other(name, reject):
    import torch
    want = _one_by_one(name, reject)
    p, cls, ext = _pieces(name, reject)
    _, ctx, _, keep = _open(name)
    try:
        d = _buffers(p, cls, ext)
        d_state = torch.zeros(12, dtype=torch.int32, device="cuda")
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        _enqueue(ctx, d, p, {1, 2, 3, 4, 5, 6}, sa.cuda_stream, sb.cuda_stream)
        ctx.nn_copy_state_device(d_state.data_ptr(), sa.cuda_stream)
        assert ctx.refine_status() == 0               # the last batch's
        assert predictor.refine_at_status(ctx) == 0   # jobs refused one by one: none (a rejected batch refuses none)
        torch.cuda.synchronize()
        got = {step: _read(d, step) for step in range(1, 7)}
        dev_state = d_state.cpu().numpy().view(np.uint32)
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    for step in range(1, 7):
        _same(got[step][0], want[step][0], f"{name} step {step}")
    assert np.array_equal(got[5][1], want[5][1]) and got[5][1].any(), f"{name} ruiSAD"
    state = {step: want[step][-1] for step in want}
    assert np.array_equal(dev_state, state[6]) and np.array_equal(after, state[6])
    assert np.array_equal(state[4], state[3]) and np.array_equal(state[5], state[3])   # neither touches the state
    n3 = len(p[2])
    if reject:
        assert got[3][0].tobytes() == _blank(n3, NN_ROW_DTYPE).tobytes()
        assert got[4][0].tobytes() == _blank(n3, RESULT_DTYPE).tobytes()
        assert np.array_equal(state[3], state[2])     # the state passed through the rejected batch
        # the batch after it is what a run without piece 3 gives: piece 4 from the state piece 2 left
        _, alone, _, keep2 = _open(name)
        try:
            alone.nn_set_state(state[2])
            rest = alone.refine(p[3])
            st = alone.nn_get_state()
        finally:
            _close(alone)
        _same(got[6][0], rest, f"{name} without piece 3")
        assert np.array_equal(state[6], st)
    else:
        assert not np.array_equal(state[3], state[2])   # the inputs batch advanced it
        assert (got[4][0]["nn_class"] == cls).all() and (got[4][0]["status"] & RES_REJECTED == 0).all()
