"""xPatternSearchFracDIF's single-PU entry point at bit depth 10, served by the resident server
kernel (csrc/fme_server.hip, k_server<10>): the 10-bit payload through the mailbox (request blocks
for small PUs, SrvBox::win / key for 16x16 and larger), the 16-bit window in LDS, both filter stages
at 14 - 10 bits of head room, the whole-PU distortion shift.

Every expected value is the C oracle's (Oracle(bit_depth=10).refine) on 416x240 synth_luma_hbd
pictures; the single calls go through test_gpu_parity._frac_single_check."""
import time

import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import JOB_BIPRED, JOB_EMI, JOB_LOSSLESS
from test_gpu_parity import _assert_same, _frac_single_check

pytestmark = pytest.mark.gpu

W, H = 416, 240
LAMBDAS = synth.LDP_LAMBDA[22]
_PICS = {}


def _pictures():
    if not _PICS:
        for k, t in zip(range(5), (7, 6, 5, 4, 0)):
            _PICS[k] = synth.synth_luma_hbd(W, H, t, 10)
        assert int(_PICS[0].max()) > 255 and int((_PICS[0] & 3).max()) == 3
    return _PICS


def _engines(pics, keys, use_hadamard=1):
    """A fresh 10-bit context and the oracle, same pictures, lambdas and keys."""
    from nnfme.runtime import FmeContext
    from oracle import Oracle
    ctx = FmeContext(use_hadamard=use_hadamard, nn_mode=1, qp=22, fast_inter_mode=1, bit_depth=10)
    orc = Oracle(use_hadamard=use_hadamard, nn_mode=1, qp=22, fast_inter_mode=1, bit_depth=10)
    for e in (ctx, orc):
        for k, v in pics.items():
            e.set_picture(k, v)
        for lid, lam in enumerate(LAMBDAS):
            e.set_lambda(lid, lam)
        if len(keys):
            e.set_keys(keys)
    orc.load_nn(weights.load_weights(22))
    return ctx, orc


def _place(jobs, i, x, y, mv, mvp):
    """Job i at (x, y) with the TZ start / integer MV mv (full-pel) and predictor mvp (quarter-pel),
    the search range by make_jobs' rule (xSetSearchRange + clipMv)."""
    sr = synth.SEARCH_RANGE << 2
    cpx = synth._clip_mv_qpel(np.int64(mvp[0]), x, W)
    cpy = synth._clip_mv_qpel(np.int64(mvp[1]), y, H)
    lt_x = synth._div4_round(synth._clip_mv_qpel(cpx - sr, x, W))
    rb_x = synth._div4_round(synth._clip_mv_qpel(cpx + sr, x, W))
    lt_y = synth._div4_round(synth._clip_mv_qpel(cpy - sr, y, H))
    rb_y = synth._div4_round(synth._clip_mv_qpel(cpy + sr, y, H))
    jobs["x"][i], jobs["y"][i] = x, y
    jobs["mvp_x"][i], jobs["mvp_y"][i] = mvp
    jobs["lt_x"][i], jobs["lt_y"][i], jobs["rb_x"][i], jobs["rb_y"][i] = lt_x, lt_y, rb_x, rb_y
    jobs["mv_x"][i] = int(np.clip(mv[0], lt_x, rb_x))
    jobs["mv_y"][i] = int(np.clip(mv[1], lt_y, rb_y))


def _shape_jobs(rng):
    """Per shape of ALL_PU_SIZES: a SATD job, a lossless (SAD) job and a bi-pred keyed job; then, per
    picture corner, an 8x8 and a 16x16 bi-pred job (one per payload route) whose integer MV points
    outside the picture, so that the window lies in the padding."""
    shapes = synth.ALL_PU_SIZES
    w = np.repeat([s[0] for s in shapes], 3)
    h = np.repeat([s[1] for s in shapes], 3)
    jobs = synth.make_jobs(rng, W, H, len(w), 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(w, h))
    jobs["flags"][1::3] = JOB_EMI | JOB_LOSSLESS
    jobs["flags"][2::3] = JOB_BIPRED
    jobs["key_offset"][2::3] = -2
    corner = synth.make_jobs(rng, W, H, 8, 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(np.tile([8, 16], 4), np.tile([8, 16], 4)))
    corner["flags"] = JOB_BIPRED
    corner["key_offset"] = -2
    for i in range(8):
        s = int(corner["w"][i])
        left, top = (i // 2) & 1, (i // 4) & 1
        x, y = (0 if left else W - s), (0 if top else H - s)
        mv = (-30 if left else 14, -21 if top else 13)
        _place(corner, i, x, y, mv, (4 * mv[0] + 3, 4 * mv[1] - 2))
    return np.concatenate([jobs, corner])


def _golden(pics, jobs, keys, orc):
    return {"jobs": jobs, "results": orc.refine(jobs), "pictures": [pics[k] for k in sorted(pics)],
            "keys": keys, "lambdas": np.asarray(LAMBDAS)}


def test_single10_first_call_is_served_by_the_server():
    """The first single call of a fresh 10-bit context, an 8x8 PU, equals the oracle and reports the
    server's device time: the call went through the mailbox (0.0 = the mailbox was never opened).
    The phase checkpoints are recorded from the first query that asks for them on (each costs the
    kernel a wall-clock read), so the four checkpoints are checked on the call after that query:
    positive and non-decreasing."""
    pics = _pictures()
    rng = np.random.default_rng(101)
    jobs = synth.make_jobs(rng, W, H, 2, 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(np.array([8, 8]), np.array([8, 8])))
    ctx, orc = _engines(pics, np.zeros(0, np.int16))
    g = _golden(pics, jobs, np.zeros(0, np.int16), orc)
    _frac_single_check(ctx, g, [0])
    us = ctx.single_last_device_us(phases=True)
    print("first call:", us)
    assert us[0] > 0, us
    _frac_single_check(ctx, g, [1])
    us = ctx.single_last_device_us(phases=True)
    print("second call:", us)
    assert us[0] > 0, us
    marks = us[1:5]
    assert all(m > 0 for m in marks) and all(b >= a for a, b in zip(marks, marks[1:])), us


@pytest.mark.parametrize("use_hadamard", [1, 0])
def test_single10_every_shape_both_payload_routes(use_hadamard):
    """Every PU shape, SATD / lossless / bi-pred keyed, with HADME on and off: the tagged route up to
    12x16 and 16x12 (1344 B), the mailbox's win / key from 16x16 (1664 B) on, 4x8 and 8x4 (two 4x4
    blocks in a four-block wave), both first-stage loops (up to 32x32, larger), the 8x8 and 4x4
    transforms, and corner PUs whose window lies in the picture's padding."""
    pics = _pictures()
    rng = np.random.default_rng(103)
    jobs = _shape_jobs(rng)
    keys = synth.make_bipred_keys(rng, jobs, pics)
    assert int(keys.max()) > 1023 and int(keys.min()) < 0   # keys outside the sample range
    ctx, orc = _engines(pics, keys, use_hadamard)
    g = _golden(pics, jobs, keys, orc)
    _frac_single_check(ctx, g, range(len(jobs)))


def _range_case(ref_plane):
    """64x64 and 8x4 bi-pred jobs against ref_plane, keys at the bi-pred extremes (-1023 and 2046)
    in 4x4 blocks, and in 2x1 blocks (finer than either transform)."""
    pics = dict(_pictures())
    pics[0] = ref_plane
    rng = np.random.default_rng(104)
    w = np.array([64, 8, 64, 8, 64, 8])
    h = np.array([64, 4, 64, 4, 64, 4])
    jobs = synth.make_jobs(rng, W, H, len(w), 4, [0], [0, 1, 2, 3], sizes=(w, h))
    jobs["flags"] = JOB_BIPRED
    off, parts = 0, []
    for i in range(len(jobs)):
        jw, jh = int(jobs["w"][i]), int(jobs["h"][i])
        yy, xx = np.mgrid[0:jh, 0:jw]
        if i < 2:
            hi = ((yy // 4) + (xx // 4)) & 1
        elif i < 4:
            hi = ((xx // 2) + yy) & 1
        else:
            hi = np.ones_like(xx) if i == 4 else np.zeros_like(xx)
        parts.append(np.where(hi == 1, 2046, -1023).astype(np.int16).reshape(-1))
        jobs["key_offset"][i] = off
        off += jw * jh
    keys = np.concatenate(parts)
    for use_hadamard in (1, 0):
        ctx, orc = _engines(pics, keys, use_hadamard)
        g = _golden(pics, jobs, keys, orc)
        _frac_single_check(ctx, g, range(len(jobs)))


def test_single10_range_checkerboard():
    """A 0 / 1023 checkerboard of period 1 (the filters' extreme outputs in both directions) under
    keys of -1023 and 2046: the first stage fits int16, |d| reaches 3069 and a 64x64 PU's sum
    approaches 2^30 before the whole-PU shift."""
    yy, xx = np.mgrid[0:H, 0:W]
    _range_case((((xx + yy) & 1) * 1023).astype(np.uint16))


def test_single10_range_vertical_stripes():
    """Vertical 0 / 1023 stripes of period 2: the horizontal filter at its extremes, the vertical one
    on constant columns."""
    yy, xx = np.mgrid[0:H, 0:W]
    _range_case((((xx >> 1) & 1) * 1023).astype(np.uint16))


def test_single10_server_lifecycle():
    """The 10-bit instance idles out and is relaunched, is stopped by a batch and relaunched after
    it, and serves NN_pred on the same context; every answer equals the oracle throughout."""
    from oracle import Oracle
    pics = _pictures()
    rng = np.random.default_rng(105)
    jobs = synth.make_jobs(rng, W, H, 64, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=0.2)
    keys = synth.make_bipred_keys(rng, jobs, pics)
    ctx, orc = _engines(pics, keys)
    g = _golden(pics, jobs, keys, orc)
    idx = list(range(0, 64, 7))
    _frac_single_check(ctx, g, idx)
    time.sleep(0.02)                                     # > the idle limit: the instance has left
    _frac_single_check(ctx, g, idx)
    _assert_same(ctx.refine(jobs), g["results"], "10-bit batch between single calls")
    _frac_single_check(ctx, g, idx)
    e, c = np.arange(1000, 9000, 1000, dtype=np.uint32), 4321
    want = Oracle().nn_class(weights.load_weights(22), e, c, 16, 8)[0]
    assert ctx.nn_pred_single(e, c, 16, 8)[0] == want
    _frac_single_check(ctx, g, idx)
    assert ctx.nn_pred_single(e, c, 16, 8)[0] == want
