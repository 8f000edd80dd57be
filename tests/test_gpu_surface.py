"""The sub-pel cost surface on the GPU (include/fme_surface.h, csrc/fme_surface.hip): fme_cost_surface /
fme_cost_surface_device against the fixtures whose distortions are the reference's own primitives
(tests/golden/surface), against the numpy restatement's costs, replayed through xPatternRefinement's
two stages against every job of the refinement goldens, against the library's own search on a
synthetic frame, and fme_hm::CostSurface through its C++ driver.  Every comparison is == on
integers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_bit_depth, load_golden
from nnfme import surface, synth
from nnfme.abi import compare_results
from nnfme.runtime import FmeContext, FmeError
from test_surface_numpy import FIXTURES, REPLAY_GOLDENS, assert_replay, fixture_surfaces, order_matters

pytestmark = pytest.mark.gpu

UNSET = 9   # a picture slot nothing is bound to


def make_ctx(g, nn_mode=0):
    ctx = FmeContext(device=0, use_hadamard=int(g["config"][0]), nn_mode=nn_mode, qp=int(g["config"][3]),
                     fast_inter_mode=int(g["config"][1]), bit_depth=golden_bit_depth(g))
    for k in range(len(g["pictures"])):
        ctx.set_picture(k, g["pictures"][k])
    for k, lam in enumerate(g["lambdas"]):
        ctx.set_lambda(k, float(lam))
    ctx.set_keys(g["keys"])
    return ctx


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    g, want = fixture_surfaces(request.param)
    ctx = make_ctx(g)
    yield g, want, ctx
    ctx.close()


def _assert_surf(got, want):
    assert got.shape == want.shape and got.dtype == surface.SURFACE_DTYPE
    for f in ("dist", "cost"):
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, (f, bad[:10], got[f][tuple(bad[:10].T)], want[f][tuple(bad[:10].T)])


def test_matches_fixture(golden):
    g, want, ctx = golden
    surf, pick = surface.cost_surface(ctx, g["jobs"])
    bad = np.argwhere(surf["dist"] != g["dist"])   # the reference's primitives
    assert bad.size == 0, (bad[:10], g["jobs"][bad[:10, 0]])
    _assert_surf(surf, want)                        # and surface_numpy's cost
    assert (pick["status"] == 0).all()


@pytest.mark.parametrize("name", REPLAY_GOLDENS)
def test_replay_reproduces_refinement_golden(name):
    """Every job: the GPU surface centred on mv_int, replayed, gives the reference's half and quarter
    offsets and its cost."""
    g = load_golden(name)
    ctx = make_ctx(g)
    try:
        surf, _ = surface.cost_surface(ctx, surface.jobs_at_results(g["jobs"], g["results"]), pick=False)
    finally:
        ctx.close()
    assert_replay(surf, g["results"])
    assert order_matters(surf).size > 0


@functools.lru_cache(maxsize=None)
def _frame():
    W, H = 416, 240
    rng = np.random.default_rng(11)
    pics = {i: synth.synth_luma(W, H, i) for i in range(5)}
    jobs = synth.make_ctu_jobs(rng, W, H, 120, 4, [0, 1, 2, 3], [0, 1, 2, 3], bipred_frac=0.1)
    keys = synth.make_bipred_keys(rng, jobs, pics)
    return pics, jobs, keys


def test_consistent_with_the_library_search():
    """A 416x240 frame with NN on: the surface at the search's pick is the search's cost, the
    minimum is not above it, the probe is the NN class's cost; the surface call leaves the NN state
    and every later refinement as they were."""
    pics, jobs, keys = _frame()
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=1, qp=22, fast_inter_mode=1)
    try:
        for k, v in pics.items():
            ctx.set_picture(k, v)
        for lid, lam in enumerate(synth.LDP_LAMBDA[22]):
            ctx.set_lambda(lid, lam)
        ctx.set_keys(keys)
        state0 = ctx.nn_get_state()
        before = ctx.refine(jobs)
        state1 = ctx.nn_get_state()
        probes = np.stack([before["nn_class"], np.full(len(jobs), surface.NO_PROBE, np.uint8)], axis=1)
        surf, pick = surface.cost_surface(ctx, surface.jobs_at_results(jobs, before), probes)
        assert (ctx.nn_get_state() == state1).all()
        ctx.nn_set_state(state0)
        after = ctx.refine(jobs)
        assert compare_results(after, before)[0] == 0 and after.tobytes() == before.tobytes()
        assert (ctx.nn_get_state() == state1).all()
    finally:
        ctx.close()
    rows = np.arange(len(jobs))
    at = surface.index(2 * before["half_x"].astype(int) + before["qtr_x"], 2 * before["half_y"].astype(int) + before["qtr_y"])
    bad = np.flatnonzero(surf["cost"][rows, at] != before["frac_cost"])
    assert bad.size == 0, (bad[:10], surf["cost"][rows, at][bad[:10]], before["frac_cost"][bad[:10]], jobs[bad[:10]])
    assert (before["nn_class"] < 49).all()
    assert (pick["probe_cost"][:, 0] == surf["cost"][rows, before["nn_class"]]).all()
    assert (pick["probe_cost"][:, 1] == surface.NO_COST).all()
    assert (pick["min_cost"] <= before["frac_cost"]).all() and (pick["min_cost"] <= pick["probe_cost"][:, 0]).all()
    rg = surface.regret(before, surf)
    assert (rg["search_cost"] == before["frac_cost"]).all() and (rg["min_cost"] == pick["min_cost"]).all()
    assert (rg["class_cost"] == pick["probe_cost"][:, 0]).all()


def test_shuffled_job_order(golden):
    """Mixed shapes side by side in one workgroup: the wave packing of groups of every size."""
    g, want, ctx = golden
    perm = np.random.default_rng(22).permutation(len(g["jobs"]))
    _assert_surf(surface.cost_surface(ctx, g["jobs"][perm], pick=False)[0], want[perm])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_group_and_workgroup_boundaries(golden, n):
    """n jobs of the 8x4 shape (4 lanes each): one group, a workgroup's last slot, a full one, one
    more (and the 8-byte tail of an odd count of rows)."""
    g, want, ctx = golden
    idx = np.resize(np.flatnonzero((g["jobs"]["w"] == 8) & (g["jobs"]["h"] == 4)), n)
    surf, pick = surface.cost_surface(ctx, g["jobs"][idx])
    _assert_surf(surf, want[idx])
    assert pick.tobytes() == surface.pick_numpy(want[idx]).tobytes()


def test_single_64x64(golden):
    """256 units on a group of 64 lanes: every lane walks four units."""
    g, want, ctx = golden
    idx = np.flatnonzero((g["jobs"]["w"] == 64) & (g["jobs"]["h"] == 64))
    assert idx.size
    for i in idx[:2]:
        _assert_surf(surface.cost_surface(ctx, g["jobs"][i:i + 1], pick=False)[0], want[i:i + 1])


def test_batch_split_anywhere_equals_the_whole(golden):
    g, want, ctx = golden
    n = len(g["jobs"])
    for cut in (1, 63, 64, 65, 129, n - 1):
        a = surface.cost_surface(ctx, g["jobs"][:cut], pick=False)[0]
        b = surface.cost_surface(ctx, g["jobs"][cut:], pick=False)[0]
        _assert_surf(np.concatenate([a, b]), want)


def test_picks_and_probes(golden):
    g, want, ctx = golden
    n = len(g["jobs"])
    rng = np.random.default_rng(3)
    probes = rng.integers(0, 49, (n, 2)).astype(np.uint8)
    probes[::3, 0] = surface.NO_PROBE
    probes[::5, 1] = surface.NO_PROBE
    _, pick = surface.cost_surface(ctx, g["jobs"], probes, surface=False)
    exp = surface.pick_numpy(want, probes)
    for f in surface.PICK_DTYPE.names:
        assert (pick[f] == exp[f]).all(), f
    assert pick.tobytes() == exp.tobytes()
    assert (pick["probe_cost"][::3, 0] == surface.NO_COST).all()
    # probe None: every probe is FME_SURF_NO_PROBE
    _, none = surface.cost_surface(ctx, g["jobs"][:70], surface=False)
    assert (none["probe"] == surface.NO_PROBE).all() and (none["probe_cost"] == surface.NO_COST).all()
    assert (none["min_idx"] == exp["min_idx"][:70]).all()


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_constructed_tie(bit_depth):
    """A flat picture makes all 49 predictions equal; with mvp 5 quarter-pels right of the centre the
    offsets dx = 2 and dx = 3 (differences -3 and -2) cost the same bits and are the least: the
    first index wins."""
    W, H = 64, 64
    flat = np.full((H, W), 1 << (bit_depth - 1), np.uint16 if bit_depth > 8 else np.uint8)
    org = flat.copy()
    org[8:24, 8:24] += 3
    job = np.zeros(1, surface.JOB_DTYPE)
    job["x"], job["y"], job["w"], job["h"] = 8, 8, 16, 16
    job["org_id"], job["ref_id"], job["lambda_id"] = 0, 1, 0
    job["mv_x"], job["mv_y"] = 2, -1
    job["mvp_x"], job["mvp_y"] = 4 * 2 + 5, 4 * -1
    job["key_offset"] = -1
    lam = 20.196
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=bit_depth)
    try:
        ctx.set_picture(0, org)
        ctx.set_picture(1, flat)
        ctx.set_lambda(0, lam)
        surf, pick = surface.cost_surface(ctx, job)
    finally:
        ctx.close()
    want = surface.surfaces_numpy({0: org, 1: flat}, np.zeros(0, np.int16), [lam], job, 1, bit_depth)
    _assert_surf(surf, want)
    assert len(set(surf["dist"][0].tolist())) == 1
    a, b = int(surface.index(2, 0)), int(surface.index(3, 0))
    c = surf["cost"][0]
    assert c[a] == c[b] == c.min() and (np.delete(c, [a, b]) > c[a]).all()
    assert pick["min_idx"][0] == a and pick["min_cost"][0] == c[a]


def _three_invalid(g):
    """The fixture's first 200 jobs with three made invalid: a bad size, an unset reference, a key
    block past the key buffer."""
    jobs = g["jobs"][:200].copy()
    bad = [17, 64, 130]
    jobs["w"][17] = 6
    jobs["ref_id"][64] = UNSET
    jobs["key_offset"][130] = len(g["keys"]) - 1
    return jobs, bad


def test_device_form_and_invalid_jobs(golden):
    import torch
    g, want, ctx = golden
    jobs = g["jobs"]
    n = len(jobs)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_surf = torch.zeros(98 * n, dtype=torch.int32, device="cuda")
    d_pick = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    surface.cost_surface_device(ctx, d_jobs, None, d_surf, d_pick, n)
    assert surface.cost_surface_invalid_count(ctx) == 0
    _assert_surf(d_surf.cpu().numpy().view(surface.SURFACE_DTYPE), want)
    assert d_pick.cpu().numpy().view(surface.PICK_DTYPE).tobytes() == surface.pick_numpy(want).tobytes()

    inv, bad = _three_invalid(g)
    m = len(inv)
    d_inv = torch.from_numpy(inv.view(np.uint8).copy()).cuda()
    d_surf2 = torch.zeros(98 * m, dtype=torch.int32, device="cuda")
    d_pick2 = torch.zeros(4 * m, dtype=torch.int32, device="cuda")
    surface.cost_surface_device(ctx, d_inv, None, d_surf2, d_pick2, m)
    assert surface.cost_surface_invalid_count(ctx) == 3
    surf = d_surf2.cpu().numpy().view(surface.SURFACE_DTYPE)
    pick = d_pick2.cpu().numpy().view(surface.PICK_DTYPE)
    exp = want[:m].copy()
    exp["dist"][bad] = exp["cost"][bad] = surface.NO_COST
    _assert_surf(surf, exp)
    assert (surf[bad].view(np.uint32) == surface.NO_COST).all()   # every word
    assert (pick["status"][bad] == 1).all() and (np.delete(pick["status"], bad) == 0).all()
    assert (pick["min_cost"][bad] == surface.NO_COST).all() and (pick["probe_cost"][bad] == surface.NO_COST).all()
    good = np.delete(np.arange(m), bad)
    assert pick[good].tobytes() == surface.pick_numpy(want[:m])[good].tobytes()
    # the context is usable afterwards, and the count is the last call's
    _assert_surf(surface.cost_surface(ctx, jobs[:100], pick=False)[0], want[:100])
    surface.cost_surface_device(ctx, d_jobs, None, d_surf, None, 50)
    assert surface.cost_surface_invalid_count(ctx) == 0


def test_host_form_rejects_invalid_batch(golden):
    g, want, ctx = golden
    inv, bad = _three_invalid(g)
    surf = np.zeros(len(inv), surface.SURFACE_DTYPE)
    pick = np.zeros(len(inv), surface.PICK_DTYPE)
    surf.view(np.uint32)[:] = 0x12345678
    pick.view(np.uint8)[:] = 0x5A
    with pytest.raises(FmeError) as e:
        surface.cost_surface(ctx, inv, out=(surf, pick))
    assert e.value.code == -1   # FME_E_INVALID
    assert (surf.view(np.uint32) == 0x12345678).all() and (pick.view(np.uint8) == 0x5A).all()   # nothing written
    for b in bad:   # each of the three alone
        with pytest.raises(FmeError) as e:
            surface.cost_surface(ctx, inv[b:b + 1])
        assert e.value.code == -1
    with pytest.raises(FmeError) as e:   # a probe that is neither a position nor FME_SURF_NO_PROBE
        surface.cost_surface(ctx, g["jobs"][:2], np.array([[0, 48], [49, 0]], np.uint8))
    assert e.value.code == -1
    with pytest.raises(FmeError) as e:   # surf and pick both null
        surface.cost_surface(ctx, g["jobs"][:4], surface=False, pick=False)
    assert e.value.code == -1
    s0, p0 = surface.cost_surface(ctx, g["jobs"][:0])   # n == 0 is accepted
    assert len(s0) == 0 and len(p0) == 0
    _assert_surf(surface.cost_surface(ctx, g["jobs"][:10], pick=False)[0], want[:10])


@pytest.mark.parametrize("name", ["surf8", "surf10"])
def test_cpp_surface_adapter(tmp_path, name):
    """fme_hm::CostSurface (include/fme_hm.hpp) on a fixture exported as raw arrays, through
    tests/cpp/test_surface_adapter.cpp compiled here against the built libraries."""
    pkg = os.path.join(ROOT, "hm16.9-nn_fme_amd")
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "test_surface_adapter")
    b = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "test_surface_adapter.cpp"), "-L", pkg, "-lfme_hm", "-lfme_amd",
                        f"-Wl,-rpath,{pkg}", "-lpthread", "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    g, want = fixture_surfaces(name)
    bd = int(g["bit_depth"][0])
    n = len(g["jobs"])
    probes = np.random.default_rng(9).integers(0, 49, (n, 2)).astype(np.uint8)
    probes[::4, 1] = surface.NO_PROBE
    np.ascontiguousarray(g["pictures"], dtype=np.uint16 if bd > 8 else np.uint8).tofile(tmp_path / "pictures.raw")
    np.ascontiguousarray(g["keys"], dtype=np.int16).tofile(tmp_path / "keys.raw")
    np.ascontiguousarray(g["lambdas"], dtype=np.float64).tofile(tmp_path / "lambdas.raw")
    np.ascontiguousarray(g["jobs"]).tofile(tmp_path / "jobs.raw")
    probes.tofile(tmp_path / "probes.raw")
    np.ascontiguousarray(want).tofile(tmp_path / "surf.raw")
    (tmp_path / "meta.txt").write_text(f"{g['pictures'].shape[2]} {g['pictures'].shape[1]} {g['pictures'].shape[0]} {n} "
                                       f"{len(g['keys'])} {len(g['lambdas'])}\n")
    p = subprocess.run([exe, str(tmp_path), str(bd), str(int(g["config"][0]))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "surface adapter ok" in p.stdout
