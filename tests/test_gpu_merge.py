"""Prediction error and merge estimation on the GPU (include/fme_merge.h, csrc/fme_merge.hip):
fme_pred_error / fme_pred_error_device / fme_merge_estimate against the fixtures from the
reference's TLibCommon (tests/golden/merge), against the C oracle's motion compensation plus the
numpy xGetHADs / SAD restatement on live data, and fme_hm::MergeEstimator through its C++ driver.
Every comparison is exact: the outputs are integers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from nnfme import merge, synth
from nnfme.abi import MC_JOB_DTYPE
from nnfme.runtime import FmeContext, FmeError
from test_merge_numpy import FIXTURES, load_merge_golden

pytestmark = pytest.mark.gpu


def make_ctx(g):
    bd, had = int(g["bit_depth"][0]), int(g["use_hadamard"][0])
    ctx = FmeContext(device=0, use_hadamard=had, nn_mode=0, bit_depth=bd)
    for k in range(len(g["luma"])):
        ctx.set_picture(k, g["luma"][k])
    for lid, lam in enumerate(g["lambdas"]):
        ctx.set_lambda(lid, float(lam))
    return ctx


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    g = load_merge_golden(request.param)
    ctx = make_ctx(g)
    yield g, ctx
    ctx.close()


def test_pred_error_matches_fixture(golden):
    g, ctx = golden
    got = merge.pred_error(ctx, g["tasks"])
    bad = np.flatnonzero(got != g["dist"])
    assert bad.size == 0, (bad[:10], got[bad[:10]], g["dist"][bad[:10]], g["tasks"][bad[:10]])


def test_pred_error_shuffled_task_order(golden):
    """Mixed shapes side by side in one workgroup: the wave packing of groups of every size."""
    g, ctx = golden
    perm = np.random.default_rng(21).permutation(len(g["tasks"]))
    got = merge.pred_error(ctx, g["tasks"][perm])
    assert np.array_equal(got, g["dist"][perm])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pred_error_group_and_wave_boundaries(golden, n):
    """n tasks of the 8x4 shape (4 lanes each): one group, a workgroup's last slot, a full one, one more."""
    g, ctx = golden
    idx = np.flatnonzero((g["tasks"]["w"] == 8) & (g["tasks"]["h"] == 4))
    idx = np.resize(idx, n)
    got = merge.pred_error(ctx, g["tasks"][idx])
    assert np.array_equal(got, g["dist"][idx])


def test_merge_estimate_matches_fixture(golden):
    g, ctx = golden
    got = merge.merge_estimate(ctx, g["reqs"])
    for f in merge.MERGE_RES_DTYPE.names:
        bad = np.flatnonzero((got[f] != g["res"][f]).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, (f, bad[:10], got[f][bad[:10]], g["res"][f][bad[:10]])


def test_empty_batches_accepted(golden):
    g, ctx = golden
    assert len(merge.pred_error(ctx, g["tasks"][:0])) == 0
    assert len(merge.merge_estimate(ctx, g["reqs"][:0])) == 0


def _three_invalid(g):
    """The fixture's first 200 tasks with three made invalid: a bad slot, a PU across the border,
    flags without a list."""
    tasks = g["tasks"][:200].copy()
    h, w = g["luma"].shape[1:]
    bad = [17, 64, 130]
    l = 0 if int(tasks["flags"][17]) & 1 else 1
    tasks["ref_id"][17, l] = 40            # an unbound slot
    tasks["x"][64] = w - int(tasks["w"][64]) + 4
    tasks["flags"][130] &= 0xFC
    return tasks, bad


def test_device_entry_point(golden):
    import torch
    g, ctx = golden
    tasks = g["tasks"]
    d_tasks = torch.from_numpy(tasks.view(np.uint8).copy()).cuda()
    d_dist = torch.zeros(len(tasks), dtype=torch.int32, device="cuda")
    merge.pred_error_device(ctx, d_tasks, d_dist, len(tasks))
    assert merge.pred_error_invalid_count(ctx) == 0
    assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), g["dist"])

    inv, bad = _three_invalid(g)
    d_inv = torch.from_numpy(inv.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(len(inv), dtype=torch.int32, device="cuda")
    merge.pred_error_device(ctx, d_inv, d_out, len(inv))
    assert merge.pred_error_invalid_count(ctx) == 3
    out = d_out.cpu().numpy().view(np.uint32)
    want = g["dist"][:len(inv)].copy()
    want[bad] = 0xFFFFFFFF
    assert np.array_equal(out, want)
    # the context is usable afterwards, and the count is the last call's
    assert np.array_equal(merge.pred_error(ctx, tasks[:100]), g["dist"][:100])
    merge.pred_error_device(ctx, d_tasks, d_dist, 50)
    assert merge.pred_error_invalid_count(ctx) == 0


def test_host_entry_point_rejects_invalid_batch(golden):
    g, ctx = golden
    inv, bad = _three_invalid(g)
    with pytest.raises(FmeError) as e:
        merge.pred_error(ctx, inv)
    assert e.value.code == -1   # FME_E_INVALID
    for b in bad:   # each of the three alone
        with pytest.raises(FmeError) as e:
            merge.pred_error(ctx, inv[b:b + 1])
        assert e.value.code == -1
    q = g["reqs"][:4].copy()
    q[2]["n_cand"], q[2]["flags"] = 0, 0   # neither a candidate nor an ME result
    with pytest.raises(FmeError) as e:
        merge.merge_estimate(ctx, q)
    assert e.value.code == -1
    assert np.array_equal(merge.pred_error(ctx, g["tasks"][:10]), g["dist"][:10])


def _random_tasks(rng, n, w, h):
    shapes = np.array(synth.ALL_PU_SIZES)
    t = np.zeros(n, merge.PE_TASK_DTYPE)
    s = shapes[rng.integers(0, len(shapes), n)]
    t["w"], t["h"] = s[:, 0], s[:, 1]
    t["x"] = rng.integers(0, (w - s[:, 0]) // 4 + 1) * 4
    t["y"] = rng.integers(0, (h - s[:, 1]) // 4 + 1) * 4
    cu = np.array([merge.cu_origin(*v) for v in zip(t["x"], t["y"], t["w"], t["h"])])
    t["cu_x"], t["cu_y"] = cu[:, 0], cu[:, 1]
    t["org_id"] = 0
    t["flags"] = rng.integers(1, 4, n) | np.where(rng.random(n) < 0.15, merge.PE_LOSSLESS, 0)
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
    """About 4,000 random tasks on a 416x240 frame.  The expected values: at 8 bits the C oracle's
    motion compensation (Oracle.mc) and the numpy xGetHADs / SAD restatement; at 10 bits, where the
    C oracle has no motion compensation, the numpy prediction restatement (tests/test_merge_numpy.py
    pins both restatements to the reference's fixtures at both depths) with a subset of the uni-pred
    tasks also checked against the oracle's orc_pred_block."""
    from oracle import Oracle
    W, H, n = 416, 240, 4000
    rng = np.random.default_rng(100 + bit_depth)
    luma = {k: (synth.synth_luma(W, H, k) if bit_depth == 8 else synth.synth_luma_hbd(W, H, k, bit_depth))
            for k in range(4)}
    tasks = _random_tasks(rng, n, W, H)
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=bit_depth)
    try:
        for k, v in luma.items():
            ctx.set_picture(k, v)
        got = merge.pred_error(ctx, tasks)
    finally:
        ctx.close()
    want = np.zeros(n, np.uint32)
    if bit_depth == 8:
        orc = Oracle(use_hadamard=1, nn_mode=0)
        flat = np.full((H // 2, W // 2), 128, np.uint8)
        pics = {k: (v, flat, flat) for k, v in luma.items()}
        y, cb, cr = np.zeros((H, W), np.uint8), flat.copy(), flat.copy()
        jobs = np.zeros(n, MC_JOB_DTYPE)
        for f in ("x", "y", "w", "h", "cu_x", "cu_y", "ref_id", "mv"):
            jobs[f] = tasks[f]
        jobs["flags"] = tasks["flags"] & 3
        for i, t in enumerate(tasks):
            orc.mc(pics, jobs[i:i + 1], y, cb, cr)
            x0, y0, w, h = int(t["x"]), int(t["y"]), int(t["w"]), int(t["h"])
            had = not int(t["flags"]) & merge.PE_LOSSLESS
            want[i] = merge.dist_numpy(luma[0][y0:y0 + h, x0:x0 + w], y[y0:y0 + h, x0:x0 + w], had, 8)
    else:
        orc = Oracle(use_hadamard=1, nn_mode=0, bit_depth=bit_depth)
        for i, t in enumerate(tasks):
            want[i] = merge.pred_error_numpy(luma, t, 1, bit_depth)
        uni = [i for i in range(n) if int(tasks[i]["flags"]) & 3 in (1, 2)][:300]
        for i in uni:
            t = tasks[i]
            l = 0 if int(t["flags"]) & 1 else 1
            pic = luma[int(t["ref_id"][l])]
            mx = min((W + 8 - int(t["cu_x"]) - 1) << 2, max((-64 - 8 - int(t["cu_x"]) + 1) * 4, int(t["mv"][l][0])))
            my = min((H + 8 - int(t["cu_y"]) - 1) << 2, max((-64 - 8 - int(t["cu_y"]) + 1) * 4, int(t["mv"][l][1])))
            p = orc.pred_block(pic, int(t["x"]), int(t["y"]), int(t["w"]), int(t["h"]), mx, my)
            assert np.array_equal(p, merge.predict_numpy(luma, t, bit_depth)), i
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]], tasks[bad[:10]])


@pytest.mark.parametrize("name", ["merge8_had", "merge10_had"])
def test_cpp_merge_adapter(tmp_path, name):
    """fme_hm::MergeEstimator (include/fme_hm.hpp) on a fixture exported as raw arrays."""
    exe = os.path.join(ROOT, "hm16.9-nn_fme_amd", "host", "test_merge_adapter")
    assert os.path.exists(exe), "build it with __graft_entry__.build() (make host-test)"
    g = load_merge_golden(name)
    bd = int(g["bit_depth"][0])
    luma = np.ascontiguousarray(g["luma"], dtype=np.uint16 if bd > 8 else np.uint8)
    luma.tofile(tmp_path / "luma.raw")
    np.ascontiguousarray(g["lambdas"], dtype=np.float64).tofile(tmp_path / "lambdas.raw")
    np.ascontiguousarray(g["reqs"]).tofile(tmp_path / "reqs.raw")
    np.ascontiguousarray(g["res"]).tofile(tmp_path / "res.raw")
    (tmp_path / "meta.txt").write_text(f"{luma.shape[2]} {luma.shape[1]} {luma.shape[0]} {len(g['reqs'])} "
                                       f"{len(g['lambdas'])}\n")
    p = subprocess.run([exe, str(tmp_path), str(bd), str(int(g["use_hadamard"][0]))], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "merge adapter ok" in p.stdout
