"""The skip-mode RD check on the GPU (include/fme_skip.h, csrc/fme_skip.hip): fme_pred_sse /
fme_pred_sse_device / fme_skip_estimate against the fixtures whose predictions are the reference's
TLibCommon (tests/golden/skip), against the oracles' motion compensation plus the numpy SSE
restatement on live data, and fme_hm::SkipEstimator through its C++ driver.  Every comparison is
exact: uint32 SSEs and distortions, == on the doubles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from nnfme import merge, skip, synth
from nnfme.abi import MC_JOB_DTYPE
from nnfme.runtime import FmeContext, FmeError
from test_skip_numpy import FIXTURES, load_skip_golden

pytestmark = pytest.mark.gpu

LUMA_ONLY = 5   # a picture slot with a luma plane and no chroma planes


def make_ctx(g):
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=int(g["bit_depth"][0]))
    for k in range(len(g["y"])):
        ctx.set_picture_yuv(k, g["y"][k], g["cb"][k], g["cr"][k])
    ctx.set_picture(LUMA_ONLY, g["y"][1])
    return ctx


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    g = load_skip_golden(request.param)
    ctx = make_ctx(g)
    yield g, ctx
    ctx.close()


def _assert_sse(got, want, tasks):
    assert got.shape == want.shape and got.dtype == np.uint32
    for c, comp in enumerate(("Y", "Cb", "Cr")):
        bad = np.flatnonzero(got[:, c] != want[:, c])
        assert bad.size == 0, (comp, bad[:10], got[bad[:10]], want[bad[:10]], tasks[bad[:10]])


def test_pred_sse_matches_fixture(golden):
    g, ctx = golden
    _assert_sse(skip.pred_sse(ctx, g["tasks"]), g["sse"], g["tasks"])
    _assert_sse(skip.pred_sse(ctx, g["req_tasks"]), g["req_sse"], g["req_tasks"])


def test_pred_sse_shuffled_task_order(golden):
    """Mixed shapes side by side in one workgroup: the wave packing of groups of every size."""
    g, ctx = golden
    perm = np.random.default_rng(22).permutation(len(g["tasks"]))
    _assert_sse(skip.pred_sse(ctx, g["tasks"][perm]), g["sse"][perm], g["tasks"][perm])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pred_sse_group_and_workgroup_boundaries(golden, n):
    """n tasks of the 8x4 shape (4 lanes each, one chroma unit wide): one group, a workgroup's last
    slot, a full one, one more."""
    g, ctx = golden
    idx = np.flatnonzero((g["tasks"]["w"] == 8) & (g["tasks"]["h"] == 4))
    idx = np.resize(idx, n)
    _assert_sse(skip.pred_sse(ctx, g["tasks"][idx]), g["sse"][idx], g["tasks"][idx])


def test_pred_sse_single_64x64(golden):
    """256 units on a group of 64 lanes: every lane walks four units."""
    g, ctx = golden
    idx = np.flatnonzero((g["tasks"]["w"] == 64) & (g["tasks"]["h"] == 64))
    for i in idx[[0, 20, 40, 63]]:   # L0, L1, bi, identical bi
        _assert_sse(skip.pred_sse(ctx, g["tasks"][i:i + 1]), g["sse"][i:i + 1], g["tasks"][i:i + 1])


def _estimate_by_slice(ctx, g, reqs=None):
    reqs = g["reqs"] if reqs is None else reqs
    got = np.zeros(len(reqs), skip.SKIP_RES_DTYPE)
    for s in range(len(g["params"])):
        m = g["req_slice"][:len(reqs)] == s
        got[m] = skip.skip_estimate(ctx, g["params"][s], reqs[m])
    return got


def test_skip_estimate_matches_fixture(golden):
    g, ctx = golden
    got = _estimate_by_slice(ctx, g)
    want = g["res"]
    for f in ("best", "best_cost", "cand_cost", "cand_dist", "cand_sse", "reserved"):
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, (f, bad[:10], got[f][bad[:10]], want[f][bad[:10]])
    assert got.tobytes() == want.tobytes()
    # the fixture holds what this checks: ties, empty masks and requests without candidates
    ev = np.array([skip.eval_mask(q) for q in g["reqs"]])
    none = got["best"] == skip.SKIP_NONE
    assert (none & (g["reqs"]["n_cand"] == 0)).any() and (none & (g["reqs"]["n_cand"] > 0)).any()
    assert (none == (ev == 0)).all() and np.isinf(got["best_cost"][none]).all()
    k = got["best"][~none].astype(np.int64)
    c = got["cand_cost"][~none]
    later = np.arange(5)[None, :] > k[:, None]
    assert ((c == c[np.arange(len(k)), k][:, None]) & later).any()   # a tie: the first of the two stays


def test_skip_estimate_without_any_candidate(golden):
    """A batch in which nothing is evaluated makes no launch and yields "none" everywhere."""
    g, ctx = golden
    q = g["reqs"][:6].copy()
    q["cand_mask"][:3] = 0
    q["n_cand"][3:] = 0
    r = skip.skip_estimate(ctx, g["params"][0], q)
    assert (r["best"] == skip.SKIP_NONE).all() and np.isinf(r["best_cost"]).all() and np.isinf(r["cand_cost"]).all()
    assert (r["cand_dist"] == skip.NO_SSE).all() and (r["cand_sse"] == skip.NO_SSE).all()


def test_empty_batches_accepted(golden):
    g, ctx = golden
    assert skip.pred_sse(ctx, g["tasks"][:0]).shape == (0, 3)
    assert len(skip.skip_estimate(ctx, g["params"][0], g["reqs"][:0])) == 0


def _three_invalid(g):
    """The fixture's first 200 tasks with three made invalid: a bad size, a reference without
    chroma planes, a block past the picture edge."""
    tasks = g["tasks"][:200].copy()
    h, w = g["y"].shape[1:]
    bad = [17, 64, 130]
    tasks["w"][17] = 6
    l = 0 if int(tasks["flags"][64]) & 1 else 1
    tasks["ref_id"][64, l] = LUMA_ONLY
    tasks["x"][130] = w - int(tasks["w"][130]) + 4
    return tasks, bad


def test_device_entry_point(golden):
    import torch
    g, ctx = golden
    tasks = g["tasks"]
    d_tasks = torch.from_numpy(tasks.view(np.uint8).copy()).cuda()
    d_sse = torch.zeros(3 * len(tasks), dtype=torch.int32, device="cuda")
    skip.pred_sse_device(ctx, d_tasks, d_sse, len(tasks))
    assert skip.pred_sse_invalid_count(ctx) == 0
    _assert_sse(d_sse.cpu().numpy().view(np.uint32).reshape(-1, 3), g["sse"], tasks)

    inv, bad = _three_invalid(g)
    d_inv = torch.from_numpy(inv.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(3 * len(inv), dtype=torch.int32, device="cuda")
    skip.pred_sse_device(ctx, d_inv, d_out, len(inv))
    assert skip.pred_sse_invalid_count(ctx) == 3
    out = d_out.cpu().numpy().view(np.uint32).reshape(-1, 3)
    want = g["sse"][:len(inv)].copy()
    want[bad] = 0xFFFFFFFF
    _assert_sse(out, want, inv)
    # the context is usable afterwards, and the count is the last call's
    _assert_sse(skip.pred_sse(ctx, tasks[:100]), g["sse"][:100], tasks[:100])
    skip.pred_sse_device(ctx, d_tasks, d_sse, 50)
    assert skip.pred_sse_invalid_count(ctx) == 0


def test_host_entry_point_rejects_invalid_batch(golden):
    g, ctx = golden
    inv, bad = _three_invalid(g)
    out = np.full((len(inv), 3), 0x12345678, np.uint32)
    with pytest.raises(FmeError) as e:
        skip.pred_sse(ctx, inv, out=out)
    assert e.value.code == -1   # FME_E_INVALID
    assert (out == 0x12345678).all()   # nothing ran, nothing was written
    for b in bad:   # each of the three alone
        with pytest.raises(FmeError) as e:
            skip.pred_sse(ctx, inv[b:b + 1])
        assert e.value.code == -1
    t = g["tasks"][:1].copy()
    t["flags"] |= 0x04   # FME_MC_WP
    with pytest.raises(FmeError) as e:
        skip.pred_sse(ctx, t)
    assert e.value.code == -1
    q = g["reqs"][:4].copy()
    q[2]["n_cand"] = 6
    with pytest.raises(FmeError) as e:
        skip.skip_estimate(ctx, g["params"][0], q)
    assert e.value.code == -1
    with pytest.raises(FmeError) as e:   # a weight outside 0..64
        skip.skip_estimate(ctx, skip.make_params(10.0, (1.0, 100.0)), g["reqs"][:4])
    assert e.value.code == -1
    _assert_sse(skip.pred_sse(ctx, g["tasks"][:10]), g["sse"][:10], g["tasks"][:10])


def _random_tasks(rng, n, w, h):
    shapes = np.array(synth.ALL_PU_SIZES)
    t = np.zeros(n, skip.SSE_TASK_DTYPE)
    s = shapes[rng.integers(0, len(shapes), n)]
    t["w"], t["h"] = s[:, 0], s[:, 1]
    t["x"] = rng.integers(0, (w - s[:, 0]) // 4 + 1) * 4
    t["y"] = rng.integers(0, (h - s[:, 1]) // 4 + 1) * 4
    cu = np.array([merge.cu_origin(*v) for v in zip(t["x"], t["y"], t["w"], t["h"])])
    t["cu_x"], t["cu_y"] = cu[:, 0], cu[:, 1]
    t["org_id"] = 0
    t["flags"] = rng.integers(1, 4, n)
    t["ref_id"] = rng.integers(1, 4, (n, 2))
    amp = np.where(rng.random(n) < 0.1, 1500, 70)[:, None, None]
    t["mv"] = (rng.integers(-1000, 1001, (n, 2, 2)) * amp) // 1000
    same = rng.random(n) < 0.1   # identical bi motion
    t["ref_id"][same, 1] = t["ref_id"][same, 0]
    t["mv"][same, 1] = t["mv"][same, 0]
    for l in range(2):   # unused lists stay zero
        unused = (t["flags"] & (1 << l)) == 0
        t["ref_id"][unused, l] = 0
        t["mv"][unused, l] = 0
    return t


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_live_against_oracle(bit_depth):
    """1,500 random tasks on a 416x240 frame with textured chroma.  The expected predictions: at 8
    bits the C oracle's motion compensation (Oracle.mc), at 10 bits, where the C oracle has none,
    the reference library's (Reference.mc, oracle/_ref); the SSEs are sse_numpy over them."""
    from oracle import REF_SO, Oracle, Reference
    if bit_depth > 8 and not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref is not built (needs the reference sources): no 10-bit motion compensation to compare with")
    W, H, n = 416, 240, 1500
    rng = np.random.default_rng(200 + bit_depth)
    pics = {}
    for k in range(4):
        if bit_depth == 8:
            pics[k] = (synth.synth_luma(W, H, k),) + tuple(synth.synth_chroma(W, H, k))
        else:
            pics[k] = (synth.synth_luma_hbd(W, H, k, bit_depth),
                       synth.synth_luma_hbd(W // 2, H // 2, k, bit_depth, seed=42),
                       synth.synth_luma_hbd(W // 2, H // 2, k, bit_depth, seed=43))
    tasks = _random_tasks(rng, n, W, H)
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=bit_depth)
    try:
        for k, v in pics.items():
            ctx.set_picture_yuv(k, *v)
        got = skip.pred_sse(ctx, tasks)
    finally:
        ctx.close()
    jobs = np.zeros(n, MC_JOB_DTYPE)
    for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv", "flags"):
        jobs[f] = tasks[f]
    dt = pics[0][0].dtype
    pred = (np.zeros((H, W), dt), np.zeros((H // 2, W // 2), dt), np.zeros((H // 2, W // 2), dt))
    if bit_depth == 8:
        orc = Oracle(use_hadamard=1, nn_mode=0)
        mc = lambda j: orc.mc(pics, j, *pred)   # noqa: E731
    else:
        ref = Reference(bit_depth=bit_depth)
        for k, v in pics.items():
            ref.set_picture_yuv(k, *v)
        mc = lambda j: ref.mc(j, *pred)   # noqa: E731
    want = np.zeros((n, 3), np.uint32)
    for i, t in enumerate(tasks):
        mc(jobs[i:i + 1])
        want[i] = skip.block_sse(pics[0], pred, t, bit_depth)
    _assert_sse(got, want, tasks)


@pytest.mark.parametrize("name", ["skip8", "skip10"])
def test_cpp_skip_adapter(tmp_path, name):
    """fme_hm::SkipEstimator (include/fme_hm.hpp) on a fixture exported as raw arrays, through
    tests/cpp/test_skip_adapter.cpp compiled here against the built libraries."""
    pkg = os.path.join(ROOT, "hm16.9-nn_fme_amd")
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "test_skip_adapter")
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "test_skip_adapter.cpp"), "-L", pkg, "-lfme_hm", "-lfme_amd",
                        f"-Wl,-rpath,{pkg}", "-lpthread", "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    g = load_skip_golden(name)
    bd = int(g["bit_depth"][0])
    dt = np.uint16 if bd > 8 else np.uint8
    for f in ("y", "cb", "cr"):
        np.ascontiguousarray(g[f], dtype=dt).tofile(tmp_path / (f + ".raw"))
    np.ascontiguousarray(g["params"]).tofile(tmp_path / "params.raw")
    np.ascontiguousarray(g["req_slice"], dtype=np.int32).tofile(tmp_path / "slice.raw")
    np.ascontiguousarray(g["reqs"]).tofile(tmp_path / "reqs.raw")
    np.ascontiguousarray(g["res"]).tofile(tmp_path / "res.raw")
    (tmp_path / "meta.txt").write_text(f"{g['y'].shape[2]} {g['y'].shape[1]} {g['y'].shape[0]} {len(g['reqs'])} "
                                       f"{len(g['params'])}\n")
    p = subprocess.run([exe, str(tmp_path), str(bd)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "skip adapter ok" in p.stdout
