"""NN-direct refinement on the GPU (include/fme_direct.h, csrc/fme_direct.hip): fme_refine_direct and
its device forms against nnfme.direct.direct_numpy, built from the same context's own ordinary
refinement (class, integer MV, EMI fields, status: pinned by the parity tests) and its own cost
surface (pinned by the surface tests), and for a seeded subset from surfaces_numpy; batch splits,
interleaving with ordinary batches on the device, rejection, the compact records, both engines of
nn_mode 2, saturated pictures with keys at the ends of their range, bound planes, the C++ adapter.
Every comparison is == on integers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_bit_depth, load_golden
from nnfme import direct, surface, weights
from nnfme.abi import (E_INVALID, E_STATE, JOB_BIPRED, JOB_DTYPE, JOB_EMI, JOB_LOSSLESS, JOB_NN_IN, MV_FIELDS,
                       MV_RESULT_DTYPE, RES_REJECTED, RESULT_DTYPE, compare_results)
from nnfme.runtime import FmeContext, FmeError
from test_direct_numpy import DEEP_GOLDENS, FIXTURES, NN_GOLDENS, subset
from test_gpu_bound_planes import bind_luma
from test_stress_oracle import LAMBDAS, hi_of, refine_case, setup

pytestmark = pytest.mark.gpu

RING = ("ring_scr3x40_fen1", "ring_b4x40_sr8_fen3")
UNSET = 9   # a picture slot nothing is bound to


def _config(g, engine=0):
    hadme, fen, nn_mode, qp = (int(v) for v in g["config"][:4])
    kw = dict(use_hadamard=hadme, nn_mode=nn_mode, qp=qp, fast_inter_mode=fen, bit_depth=golden_bit_depth(g),
              nn_engine=engine)
    if "net" in g:
        kw["net"] = weights.case_net(str(g["net"]))
    return kw


def _open(name, engine=0, bind=None):
    """(fixture, context set up as the fixture's own GPU test does, its refinement jobs, what must stay
    alive while the context is used).  bind: a geometry of test_gpu_bound_planes instead of set_picture."""
    import torch
    g = load_golden(name)
    ctx = FmeContext(**_config(g, engine))
    keep = []
    for i, p in enumerate(g["pictures"]):
        if bind:
            bind_luma(ctx, keep, i, p, bind)
        else:
            ctx.set_picture(i, p)
    for i, lam in enumerate(g["lambdas"]):
        ctx.set_lambda(i, float(lam))
    if g["keys"].size:
        ctx.set_keys(g["keys"])
    jobs = g["jobs"]
    if name in RING:   # the backups' input path: FME_JOB_NN_IN jobs read the bound rows
        jobs = g["refine_jobs"]
        rows = torch.from_numpy(np.ascontiguousarray(g["nn_in"]).view(np.uint8).copy()).cuda()
        ctx.set_nn_inputs(rows.data_ptr(), len(g["nn_in"]))
        keep.append(rows)
    return g, ctx, np.ascontiguousarray(jobs), keep


def _close(ctx):
    import torch
    torch.cuda.synchronize()
    ctx.set_nn_inputs(None)
    ctx.close()


@functools.lru_cache(maxsize=None)
def expected(name, engine=0):
    """(the records a direct batch over the fixture must give from a reset state, the NN state after
    it, the ordinary refinement's records), computed once and shared (read only)."""
    g, ctx, jobs, keep = _open(name, engine)
    try:
        ref = ctx.refine(jobs)
        state = ctx.nn_get_state()
        surf, _ = surface.cost_surface(ctx, surface.jobs_at_results(jobs, ref), pick=False)
    finally:
        _close(ctx)
    exp = direct.direct_numpy(jobs, ref, surf, g["lambdas"])
    for a in (exp, state, ref, surf):
        a.setflags(write=False)
    return exp, state, ref, surf


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    for f in got.dtype.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, (what, f, bad[:10], got[f][bad[:10]], want[f][bad[:10]])
    assert got.tobytes() == want.tobytes(), what


def _upload(jobs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(jobs).view(np.uint8).copy()).cuda()


def _records(n, dtype=RESULT_DTYPE, fill=0xA5):
    import torch
    return torch.full((n * dtype.itemsize,), fill, dtype=torch.uint8, device="cuda")


def _host(t, dtype=RESULT_DTYPE):
    return t.cpu().numpy().view(dtype)


# ---- 1. every fixture, every field ----------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES + RING)
def test_direct_equals_direct_numpy(name):
    exp, state, ref, surf = expected(name)
    g, ctx, jobs, keep = _open(name)
    try:
        got = direct.refine_direct(ctx, jobs)
        assert ctx.refine_status() == 0
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    assert compare_results(ref, g["results"])[0] == 0   # the ordinary run is the fixture's (the parity tests' claim)
    _same(got, exp, name)
    assert np.array_equal(got["status"], ref["status"] | direct.RES_NN_DIRECT)
    assert np.array_equal(after, state)
    assert np.array_equal(got["frac_cost"], surface.regret(ref, surf)["class_cost"])
    if name in RING:
        nn_in, bi = (jobs["flags"] & JOB_NN_IN) != 0, (jobs["flags"] & JOB_BIPRED) != 0
        assert nn_in.sum() > 100 and (bi & ~nn_in).sum() > 0   # rows, and bi-pred jobs that reuse the last class
    else:
        assert ((jobs["flags"] & JOB_EMI) == 0).any() and ((jobs["flags"] & JOB_LOSSLESS) != 0).any()
        # the seeded subset of the CPU test: the surfaces restated in numpy instead of the GPU's
        _, idx, s = subset(name)
        want = direct.direct_numpy(jobs[idx], ref[idx], s, g["lambdas"])
        _same(got[idx], want, name + " subset")


def test_request_checks_on_a_context():
    g, ctx, jobs, keep = _open(NN_GOLDENS[0])
    off = FmeContext(use_hadamard=1, nn_mode=0, qp=22, fast_inter_mode=1)
    try:
        lib = direct.bind(ctx.lib)
        assert len(direct.refine_direct(ctx, jobs[:0])) == 0                  # n == 0 returns 0
        assert lib.fme_refine_direct_device(ctx.h, None, None, 0, None) == 0
        assert lib.fme_refine_direct_mv_device(ctx.h, None, None, 0, None) == 0
        assert lib.fme_refine_direct_device(ctx.h, None, None, 4, None) == E_INVALID
        assert lib.fme_refine_direct(ctx.h, None, None, -1, None) == E_INVALID
        with pytest.raises(FmeError) as e:
            direct.last_ms(ctx)                                                # no profiled direct batch yet
        assert e.value.code == E_STATE
        for k, p in enumerate(g["pictures"]):
            off.set_picture(k, p)
        for k, lam in enumerate(g["lambdas"]):
            off.set_lambda(k, float(lam))
        off.set_keys(g["keys"])
        with pytest.raises(FmeError) as e:
            direct.refine_direct(off, jobs[:8])                                # nn_mode 0: no class
        assert e.value.code == E_STATE
        d_jobs, d_res = _upload(jobs[:8]), _records(8)
        assert lib.fme_refine_direct_device(off.h, d_jobs.data_ptr(), d_res.data_ptr(), 8, None) == E_STATE
        assert lib.fme_refine_direct_mv_device(off.h, d_jobs.data_ptr(), d_res.data_ptr(), 8, None) == E_STATE
        assert (_host(d_res, np.dtype("u1")) == 0xA5).all()                    # nothing written
        assert len(off.refine(jobs[:8])) == 8                                  # the ordinary path is untouched
        ctx.set_profiling(True)
        direct.refine_direct(ctx, jobs[:200])
        ms = direct.last_ms(ctx)
        assert set(ms) == set(direct.LAST_MS_NAMES) and all(v > 0 for v in ms.values())
        assert ms["batch"] >= ms["emi"] + ms["class"] + ms["evaluation"] - 1e-3
    finally:
        off.close()
        _close(ctx)


# ---- 2. split anywhere ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fen3_qp27_nn", "main10_ra_qp37_nn", "deep_scr3x40_qp22"])
def test_split_batches_carry_nn_state(name):
    exp, state, _, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    rng = np.random.default_rng(77)
    cuts = sorted({0, 1, 7, 64, n - 5, n, *(int(v) for v in rng.integers(1, n, 4))})
    try:
        parts = [direct.refine_direct(ctx, jobs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    _same(np.concatenate(parts), exp, name + " split")
    assert np.array_equal(after, state)


# ---- 3. interleaved with ordinary batches on the device ---------------------------------------------------
def _five(n, seed):
    rng = np.random.default_rng(seed)
    cuts = [0, *sorted(int(v) for v in rng.choice(np.arange(64, n - 64), 4, replace=False)), n]
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("second_stream", [False, True])
@pytest.mark.parametrize("name", ["ldp_qp22_hadme_fen1_nn", "main10_fen3_qp27_nn"])
def test_interleaved_with_ordinary_batches_without_host_sync(name, second_stream):
    import torch
    exp, state, ref, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    parts = _five(len(jobs), 5)
    try:
        # the same five calls made synchronously
        sync = [direct.refine_direct(ctx, jobs[a:b]) if k & 1 else ctx.refine(jobs[a:b]) for k, (a, b) in enumerate(parts)]
        assert np.array_equal(ctx.nn_get_state(), state)
        ctx.nn_reset()
        d_jobs = [_upload(jobs[a:b]) for a, b in parts]
        d_res = [_records(b - a) for a, b in parts]
        d_state = torch.zeros(12, dtype=torch.int32, device="cuda")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(parts):
            if k & 1:
                s = s2 if second_stream else s1
                direct.refine_direct_device(ctx, d_jobs[k], d_res[k], b - a, s.cuda_stream)
            else:
                ctx.refine_device(d_jobs[k].data_ptr(), d_res[k].data_ptr(), b - a, s1.cuda_stream)
        ctx.nn_copy_state_device(d_state.data_ptr(), s1.cuda_stream)
        assert ctx.refine_status() == 0
        torch.cuda.synchronize()
        got = [_host(t) for t in d_res]
        dev_state = d_state.cpu().numpy().view(np.uint32)
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    for k, (a, b) in enumerate(parts):
        _same(got[k], sync[k], f"{name} batch {k}")
        if k & 1:
            _same(got[k], exp[a:b], f"{name} direct batch {k}")
        else:
            assert compare_results(got[k], ref[a:b])[0] == 0
    # all five carry the classes (and stale / uninit bits) of one uninterrupted ordinary run
    allr = np.concatenate(got)
    assert np.array_equal(allr["nn_class"], ref["nn_class"])
    assert np.array_equal(allr["status"] & ~np.uint16(direct.RES_NN_DIRECT), ref["status"])
    assert np.array_equal(after, state) and np.array_equal(dev_state, state)


# ---- 4. device rejection ---------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("w", 20), ("ref_id", UNSET), ("key_offset", 10 ** 8)])
def test_device_rejection_leaves_the_state(field, value):
    name = "qp32_nn"
    g, ctx, jobs, keep = _open(name)
    a, b = 200, 400
    assert b < len(jobs)
    bad = jobs[a:b].copy()
    bad[field][17] = value
    try:
        first = ctx.refine(jobs[:a])
        st = ctx.nn_get_state()
        d_bad, d_res, d_mv = _upload(bad), _records(b - a), _records(b - a, MV_RESULT_DTYPE)
        direct.refine_direct_device(ctx, d_bad, d_res, b - a)
        assert ctx.refine_status() == 1
        r = _host(d_res)
        assert ((r["status"] & RES_REJECTED) != 0).all()
        assert np.array_equal(ctx.nn_get_state(), st)
        direct.refine_direct_mv_device(ctx, d_bad, d_mv, b - a)
        assert ctx.refine_status() == 1
        assert ((_host(d_mv, MV_RESULT_DTYPE)["status"] & RES_REJECTED) != 0).all()
        assert np.array_equal(ctx.nn_get_state(), st)
        with pytest.raises(FmeError) as e:   # the host form: FME_E_INVALID, nothing computed
            direct.refine_direct(ctx, bad)
        assert e.value.code == E_INVALID
        assert np.array_equal(ctx.nn_get_state(), st)
        rest = ctx.refine(jobs[a:])          # the next ordinary batch gives the fixture's results
        assert ctx.refine_status() == 0
    finally:
        _close(ctx)
    assert compare_results(np.concatenate([first, rest]), g["results"])[0] == 0


# ---- 5. the compact records ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ra_qp27_nn", "main10_ldp_qp22_hadme_fen1_nn", "deep_master_qp22"])
def test_mv_device_equals_the_full_records(name):
    exp, state, _, _ = expected(name)
    g, ctx, jobs, keep = _open(name)
    n = len(jobs)
    try:
        d_jobs, d_mv = _upload(jobs), _records(n, MV_RESULT_DTYPE)
        direct.refine_direct_mv_device(ctx, d_jobs, d_mv, n)
        assert ctx.refine_status() == 0
        mv = _host(d_mv, MV_RESULT_DTYPE)
        after = ctx.nn_get_state()
        # in two batches, the second in the other slot's internal records
        ctx.nn_reset()
        d_mv2 = _records(n, MV_RESULT_DTYPE)
        direct.refine_direct_mv_device(ctx, d_jobs, d_mv2, 333)
        direct.refine_direct_mv_device(ctx, d_jobs.data_ptr() + 333 * JOB_DTYPE.itemsize,
                                       d_mv2.data_ptr() + 333 * MV_RESULT_DTYPE.itemsize, n - 333)
        assert ctx.refine_status() == 0
        mv2 = _host(d_mv2, MV_RESULT_DTYPE)
    finally:
        _close(ctx)
    for f in MV_FIELDS:
        assert np.array_equal(mv[f], exp[f]), f
    assert (mv["reserved"] == 0).all()
    assert mv.tobytes() == direct.mv_records(exp).tobytes() == mv2.tobytes()
    assert np.array_equal(after, state)


# ---- 6. the MFMA engine of nn_mode 2 ------------------------------------------------------------------
def test_mfma_engine_records_follow_their_class():
    name = "deep_scr3x40_qp22"
    exact, _, _, _ = expected(name)
    exp, state, ref, _ = expected(name, 1)   # from the MFMA engine's own ordinary run
    g, ctx, jobs, keep = _open(name, 1)
    try:
        got = direct.refine_direct(ctx, jobs)
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    _same(got, exp, name + " MFMA")          # every record is direct_numpy's for the class it reports
    assert np.array_equal(after, state)
    same = got["nn_class"] == exact["nn_class"]
    assert same.mean() >= 0.99               # (test_deep_nn.py's tolerance)
    assert got[same].tobytes() == exact[same].tobytes()


# ---- 7. hard content ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hadme", [1, 0])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["checker1", "binary", "flat", "twolevel"])
def test_saturated_pictures_and_extreme_keys(kind, bd, hadme):
    pics, jobs, keys = refine_case(kind, bd)
    hi = hi_of(bd)
    assert int(keys.min()) == -hi and int(keys.max()) == 2 * hi   # |d| reaches 2 hi through the Hadamard
    jobs = jobs.copy()
    jobs["lambda_id"][::5] = LAMBDAS.index(0.0)                    # lambda 0 on every fifth job
    ctx = FmeContext(bit_depth=bd, use_hadamard=hadme, nn_mode=1, qp=22, fast_inter_mode=1)
    try:
        setup(ctx, pics, keys)
        ref = ctx.refine(jobs)
        state = ctx.nn_get_state()
        surf, _ = surface.cost_surface(ctx, surface.jobs_at_results(jobs, ref), pick=False)
        ctx.nn_reset()
        got = direct.refine_direct(ctx, jobs)
        assert ctx.refine_status() == 0
        after = ctx.nn_get_state()
    finally:
        ctx.close()
    _same(got, direct.direct_numpy(jobs, ref, surf, LAMBDAS), f"{kind} {bd} HADME {hadme}")
    assert np.array_equal(after, state)
    assert (jobs["lambda_id"] == LAMBDAS.index(0.0)).any() and ((jobs["flags"] & JOB_LOSSLESS) != 0).any()


# ---- 8. bound planes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geom", [("fen3_qp27_nn", "C"), ("main10_fen3_qp27_nn", "C"), ("qp37_nn", "B")])
def test_bound_planes_with_padded_strides(name, geom):
    exp, state, _, _ = expected(name)
    g, ctx, jobs, keep = _open(name, bind=geom)
    try:
        got = direct.refine_direct(ctx, jobs)
        after = ctx.nn_get_state()
    finally:
        _close(ctx)
    _same(got, exp, f"{name} geometry {geom}")
    assert np.array_equal(after, state)


# ---- 9. the C++ adapter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ldp_qp22_hadme_fen1_nn", "main10_ldp_qp22_hadme_fen1_nn"])
def test_cpp_direct_adapter(tmp_path, name):
    """fme_hm::CtuRowBatcher with SearchConfig::nnDirect (include/fme_hm.hpp) on a fixture exported as raw
    arrays, through tests/cpp/test_direct_adapter.cpp compiled here against the built libraries."""
    pkg = os.path.join(ROOT, "hm16.9-nn_fme_amd")
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "test_direct_adapter")
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "test_direct_adapter.cpp"), "-L", pkg, "-lfme_hm", "-lfme_amd",
                        f"-Wl,-rpath,{pkg}", "-lpthread", "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    exp, _, _, _ = expected(name)
    g = load_golden(name)
    bd = golden_bit_depth(g)
    n = len(g["jobs"])
    np.ascontiguousarray(g["pictures"], dtype=np.uint16 if bd > 8 else np.uint8).tofile(tmp_path / "pictures.raw")
    np.ascontiguousarray(g["keys"], dtype=np.int16).tofile(tmp_path / "keys.raw")
    np.ascontiguousarray(g["lambdas"], dtype=np.float64).tofile(tmp_path / "lambdas.raw")
    np.ascontiguousarray(g["jobs"]).tofile(tmp_path / "jobs.raw")
    np.ascontiguousarray(exp).tofile(tmp_path / "expected.raw")
    (tmp_path / "meta.txt").write_text(f"{g['pictures'].shape[2]} {g['pictures'].shape[1]} {g['pictures'].shape[0]} {n} "
                                       f"{len(g['keys'])} {len(g['lambdas'])}\n")
    hadme, fen, _, qp = (int(v) for v in g["config"][:4])
    p = subprocess.run([exe, str(tmp_path), str(bd), str(hadme), str(fen), str(qp)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "direct adapter ok" in p.stdout
