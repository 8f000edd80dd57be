"""Bound device planes with padded strides and offset origins (fme_bind_picture_device,
fme_bind_picture_chroma_device: the zero-copy route of include/fme.h).

Every other GPU test hands the kernels planes with stride == width at the start of an allocation, so
every row they have seen starts dword aligned and a read past a row's end lands in the next row.
Here each picture of an existing fixture - the originals too - lies inside a larger device tensor
filled with seeded random samples (at 10 bits over the whole uint16 range, far above 1023), at an
origin and a row pitch that select each alignment path:

  A  the encoder's layout (HM's TComPicYuv: margins 80 x 16, stride W + 160; chroma halved):
     every row at least dword aligned (luma 16-byte aligned where W is a multiple of 16), only the
     pitch differs from the width;
  B  dword aligned only: origin 4 samples in, stride W + 12, so the rows walk through the 16-byte
     phases; chroma 2 samples in with stride W/2 + 6, at 8 bits only 2-byte aligned, so the chroma
     paths are the per-sample ones while the luma paths are the dword ones;
  C  sample aligned only: at 8 bits slot k lies 1 + k % 3 samples in with the odd stride W + 3, so
     rows take all four byte phases; at 10 bits 1 sample in with stride W + 1; chroma 1 sample in
     with stride W/2 + 1.  No plane has dword rows;
  D1 / D2  luma as A with chroma as C, and luma as C with chroma as A (where chroma is read).

The expectations are the fixtures' own (tests/golden) and, for the producers, the oracle the
existing tests compare with.  A pitch used as a width, a clamp against the wrong bound, an
alignment branch that computes something else or a read outside width x height changes a result:
the surroundings are random.  The host counterpart (FmeContext.set_picture / set_picture_chroma on
row-strided numpy views) is at the end."""
import numpy as np
import pytest

from conftest import golden_bit_depth, load_golden

SLACK = 16   # samples after the last row of an embedded plane's tensor

GEOMETRIES = ("A", "B", "C")
GEOMETRIES_YUV = ("A", "B", "C", "D1", "D2")
_LUMA_AS = {"A": "A", "B": "B", "C": "C", "D1": "A", "D2": "C"}
_CHROMA_AS = {"A": "A", "B": "B", "C": "C", "D1": "C", "D2": "A"}


def luma_geometry(geom, width, bit_depth, slot):
    """(mx, my, stride) in samples of picture slot `slot`'s luma plane in geometry `geom`."""
    kind = _LUMA_AS[geom]
    if kind == "A":
        return 80, 16, width + 160
    if kind == "B":
        return 4, 4, width + 12
    if bit_depth == 8:
        return 1 + slot % 3, 2, width + 3
    return 1, 2, width + 1


def chroma_geometry(geom, cwidth):
    """(mx, my, stride) of the two chroma planes: half the luma margins."""
    kind = _CHROMA_AS[geom]
    if kind == "A":
        return 40, 8, cwidth + 80
    if kind == "B":
        return 2, 2, cwidth + 6
    return 1, 1, cwidth + 1


def poison(n, dtype, seed):
    """n seeded random samples over the dtype's whole range (uint16: mostly above 10 bits)."""
    return np.random.default_rng(seed).integers(0, 1 << (8 * np.dtype(dtype).itemsize), n, dtype=dtype)


def plane_view(buf, origin, stride, height, width):
    """The height x width view of the 1-D sample array buf whose sample (0, 0) is buf[origin]."""
    item = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[origin:], shape=(height, width), strides=(stride * item, item))


def embed_numpy(plane, mx, my, stride, seed):
    """plane inside (H + 2 my) * stride + SLACK poison samples, its sample (0, 0) at row my, column
    mx of the stride-wide rows: (the 1-D array, the origin's index)."""
    plane = np.asarray(plane)
    h, w = plane.shape
    assert plane.dtype in (np.uint8, np.uint16) and mx >= 0 and my >= 0 and mx + w <= stride
    buf = poison((h + 2 * my) * stride + SLACK, plane.dtype, seed)
    origin = my * stride + mx
    plane_view(buf, origin, stride, h, w)[...] = plane
    return buf, origin


def embed(plane, mx, my, stride, seed):
    """embed_numpy's array as one device tensor: (pointer to sample (0, 0), stride in samples, the
    tensor).  The caller keeps the tensor alive while the plane is bound."""
    import torch
    buf, origin = embed_numpy(plane, mx, my, stride, seed)
    t = torch.from_numpy(buf.view(np.uint8)).cuda()
    assert t.data_ptr() % 256 == 0   # the geometries' alignments count from an aligned allocation
    return t.data_ptr() + origin * buf.itemsize, stride, t


def bind_luma(ctx, keep, slot, plane, geom):
    h, w = plane.shape
    mx, my, stride = luma_geometry(geom, w, 8 if plane.dtype == np.uint8 else 10, slot)
    ptr, stride, t = embed(plane, mx, my, stride, 7000 + slot)
    keep.append(t)
    ctx.bind_picture_device(slot, ptr, stride, w, h)


def bind_chroma(ctx, keep, slot, cb, cr, geom):
    assert cb.shape == cr.shape
    mx, my, stride = chroma_geometry(geom, cb.shape[1])
    pb, _, tb = embed(cb, mx, my, stride, 8000 + slot)
    pr, _, tr = embed(cr, mx, my, stride, 9000 + slot)
    keep += [tb, tr]
    ctx.bind_picture_chroma_device(slot, pb, pr, stride)


def picture_binder(geom, keep):
    """bind(ctx, pics) for the producers' set-up: every luma plane of {slot: plane} bound in geom."""
    def bind(ctx, pics):
        for k, v in pics.items():
            bind_luma(ctx, keep, k, v, geom)
    return bind


def _sample_dtype(bit_depth):
    return np.uint16 if bit_depth > 8 else np.uint8


# ---- the helper, on numpy arrays ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_embed_places_the_plane_in_poison(dtype):
    bd = 8 if dtype == np.uint8 else 10
    W, H = 24, 10
    plane = np.random.default_rng(1).integers(0, 1 << bd, (H, W), dtype=dtype)
    cases = [luma_geometry(g, W, bd, slot) for g in GEOMETRIES for slot in range(3)]
    cases += [chroma_geometry(g, W) for g in GEOMETRIES]
    assert len({c[2] - W for c in cases}) >= 5
    for seed, (mx, my, stride) in enumerate(cases):
        buf, origin = embed_numpy(plane, mx, my, stride, seed)
        assert buf.dtype == dtype and buf.ndim == 1 and len(buf) == (H + 2 * my) * stride + SLACK
        assert origin == my * stride + mx
        assert np.array_equal(plane_view(buf, origin, stride, H, W), plane)
        outside = np.ones(len(buf), bool)
        for r in range(H):
            outside[origin + r * stride:origin + r * stride + W] = False
        assert outside.sum() == len(buf) - W * H
        want = poison(len(buf), dtype, seed)
        assert np.array_equal(buf[outside], want[outside])
        # what surrounds the plane is not a picture: every byte phase of the rows is random, and at
        # 10 bits most of it is no 10-bit sample
        assert len(np.unique(buf[outside])) > min(100, outside.sum() // 2)
        if dtype == np.uint16:
            assert (buf[outside] > 1023).mean() > 0.9
    a, _ = embed_numpy(plane, 1, 1, W + 1, 5)
    b, _ = embed_numpy(plane, 1, 1, W + 1, 6)
    assert not np.array_equal(a, b)


def test_geometries_select_the_alignment_paths():
    """What each geometry promises, from the byte offsets alone (the allocation is 256-byte aligned)."""
    def phases(mx, my, stride, item, rows=8):
        return {((my + r) * stride + mx) * item % 16 for r in range(rows)}

    for W in (128, 160, 168, 192, 384):
        for bd, item in ((8, 1), (10, 2)):
            for slot in range(6):
                a = phases(*luma_geometry("A", W, bd, slot), item) | phases(*chroma_geometry("A", W // 2), item)
                assert all(p % 4 == 0 for p in a)
                if W % 16 == 0:
                    assert phases(*luma_geometry("A", W, bd, slot), item) == {0}
                b = phases(*luma_geometry("B", W, bd, slot), item)
                assert all(p % 4 == 0 for p in b) and len(b) > 1
                c = phases(*luma_geometry("C", W, bd, slot), item)
                if bd == 8:   # all four byte phases of a dword
                    assert {p % 4 for p in c} == {0, 1, 2, 3}
                else:         # rows alternate between a dword and the middle of one
                    assert {p % 4 for p in c} == {0, 2}
                assert luma_geometry("C", W, bd, slot)[2] % 2 == 1
            assert {luma_geometry("C", W, 8, k)[0] for k in range(6)} == {1, 2, 3}
        cb = phases(*chroma_geometry("B", W // 2), 1)
        assert all(p % 2 == 0 for p in cb) and any(p % 4 for p in cb)   # 8 bits: 2-byte aligned only
        assert chroma_geometry("C", W // 2)[2] % 2 == 1
    assert (_LUMA_AS["D1"], _CHROMA_AS["D1"], _LUMA_AS["D2"], _CHROMA_AS["D2"]) == ("A", "C", "C", "A")


# ---- which picture borders the fixtures' windows cross -----------------------------------------------
REFINE_FIXTURES = ("ldp_qp22_hadme_fen1_nn", "sad_fen0_nnoff", "main10_ldp_qp22_hadme_fen1_nn")
TZ_FIXTURES = ("tz_far_fen0_sr32", "tz_ldp_fen1", "tz10_far_fen0_sr32", "tz_enhanced_fen1")
# per border, an integer-search fixture in which at least 8 jobs' best window crosses it
TZ_BORDER_FIXTURE = {"left": "tz_ldp_fen1", "right": "tz_ldp_fen1", "top": "tz_far_fen0_sr32", "bottom": "tz_ldp_fen1"}
BORDERS = ("left", "right", "top", "bottom")


def border_crossings(jobs, mv_x, mv_y, margin, width, height):
    """{border: jobs whose window - the PU displaced by the full-pel MV, `margin` samples more on
    every side - reaches outside the picture there}."""
    x0 = jobs["x"].astype(np.int64) + mv_x.astype(np.int64) - margin
    y0 = jobs["y"].astype(np.int64) + mv_y.astype(np.int64) - margin
    x1 = x0 + jobs["w"].astype(np.int64) + 2 * margin
    y1 = y0 + jobs["h"].astype(np.int64) + 2 * margin
    return {"left": int((x0 < 0).sum()), "right": int((x1 > width).sum()), "top": int((y0 < 0).sum()),
            "bottom": int((y1 > height).sum())}


def refine_crossings(g):
    """The refinement's window: the PU at its integer MV, 4 samples around it (the 8-tap filters)."""
    h, w = g["pictures"].shape[1:]
    return border_crossings(g["jobs"], g["jobs"]["mv_x"], g["jobs"]["mv_y"], 4, w, h)


def tz_crossings(g):
    """The integer search's window at the MV it returns (a candidate it has certainly loaded)."""
    h, w = g["pictures"].shape[1:]
    return border_crossings(g["jobs"], g["mv_x"], g["mv_y"], 0, w, h)


@pytest.mark.parametrize("case", REFINE_FIXTURES)
def test_refine_fixtures_cross_every_border(case):
    n = refine_crossings(load_golden(case))
    assert all(n[b] >= 8 for b in BORDERS), n


def test_tz_fixtures_cross_every_border():
    n = {case: tz_crossings(load_golden(case)) for case in TZ_FIXTURES}
    for case in TZ_FIXTURES:
        assert all(n[case][b] >= 1 for b in BORDERS), (case, n[case])
    for b in BORDERS:
        assert n[TZ_BORDER_FIXTURE[b]][b] >= 8, (b, n)


# ---- refinement: k_search_lane, k_search_lane10, the NN tail --------------------------------------------
def _bind_pictures(ctx, keep, pictures, geom):
    for k in range(len(pictures)):
        bind_luma(ctx, keep, k, pictures[k], geom)


def _refine_ctx(g, keep, geom):
    from nnfme.runtime import FmeContext
    hadme, fen, nn_mode, qp = (int(v) for v in g["config"])
    ctx = FmeContext(use_hadamard=hadme, nn_mode=nn_mode, qp=qp, fast_inter_mode=fen, bit_depth=golden_bit_depth(g))
    _bind_pictures(ctx, keep, g["pictures"], geom)
    for i, lam in enumerate(g["lambdas"]):
        ctx.set_lambda(i, float(lam))
    if g["keys"].size:
        ctx.set_keys(g["keys"])
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("case", REFINE_FIXTURES)
def test_refine(case, geom):
    from test_gpu_parity import _assert_same
    g = load_golden(case)
    n = refine_crossings(g)
    assert all(n[b] >= 8 for b in BORDERS), n
    keep = []
    ctx = _refine_ctx(g, keep, geom)
    try:
        res = ctx.refine(g["jobs"])
        assert ctx.refine_status() == 0
    finally:
        ctx.close()
    _assert_same(res, g["results"], f"{case} in geometry {geom}")


# ---- integer search: the staged tiles, the raster, the candidate windows -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("case", TZ_FIXTURES)
def test_integer_search(case, geom):
    import torch
    from nnfme.abi import JOB_DTYPE, TZ_EXT2_DTYPE
    from nnfme.runtime import FmeContext
    g = load_golden(case)
    n = tz_crossings(g)
    assert all(n[b] >= 1 for b in BORDERS), n
    keep = []
    ctx = FmeContext(nn_mode=0, fast_inter_mode=int(g["config"][0]), bit_depth=golden_bit_depth(g))
    try:
        _bind_pictures(ctx, keep, g["pictures"], geom)
        for i, lam in enumerate(g["lambdas"]):
            ctx.set_lambda(i, float(lam))
        if g["keys"].size:
            ctx.set_keys(g["keys"])
        if g["ext"].dtype.itemsize == TZ_EXT2_DTYPE.itemsize:   # FastSearch 0 / 3: the device entry point
            dj = torch.from_numpy(g["jobs"].view(np.uint8).copy()).cuda()
            de = torch.from_numpy(np.ascontiguousarray(g["ext"]).view(np.uint8).copy()).cuda()
            ds = torch.zeros(len(g["jobs"]), dtype=torch.int32, device="cuda")
            ctx.integer_search2_device(dj.data_ptr(), de.data_ptr(), ds.data_ptr(), len(g["jobs"]),
                                       torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            jobs, sad = dj.cpu().numpy().view(JOB_DTYPE), ds.cpu().numpy().view(np.uint32)
        else:   # a rejected job makes the host form raise
            jobs, sad = ctx.integer_search(g["jobs"], g["ext"])
    finally:
        ctx.close()
    bad = (jobs["mv_x"] != g["mv_x"]) | (jobs["mv_y"] != g["mv_y"]) | (sad != g["sad"])
    assert not bad.any(), f"{case} in geometry {geom}: {int(bad.sum())} of {len(bad)} jobs differ " \
                          f"(first {int(np.flatnonzero(bad)[0])})"


# ---- cost surface ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("case", ["surf8", "surf8_sad", "surf10"])
def test_cost_surface(case, geom):
    from nnfme import surface
    from nnfme.runtime import FmeContext
    from test_surface_numpy import fixture_surfaces
    g, want = fixture_surfaces(case)
    keep = []
    ctx = FmeContext(device=0, use_hadamard=int(g["config"][0]), nn_mode=0, qp=int(g["config"][3]),
                     fast_inter_mode=int(g["config"][1]), bit_depth=golden_bit_depth(g))
    try:
        _bind_pictures(ctx, keep, g["pictures"], geom)
        for k, lam in enumerate(g["lambdas"]):
            ctx.set_lambda(k, float(lam))
        ctx.set_keys(g["keys"])
        surf, pick = surface.cost_surface(ctx, g["jobs"])
        assert surface.cost_surface_invalid_count(ctx) == 0
    finally:
        ctx.close()
    bad = np.argwhere(surf["dist"] != g["dist"])   # the reference's primitives
    assert bad.size == 0, (bad[:10], g["jobs"][bad[:10, 0]])
    for f in ("dist", "cost"):                       # and surface_numpy's cost
        bad = np.argwhere(surf[f] != want[f])
        assert bad.size == 0, (f, bad[:10], surf[f][tuple(bad[:10].T)], want[f][tuple(bad[:10].T)])
    assert (pick["status"] == 0).all()
    assert pick.tobytes() == surface.pick_numpy(want).tobytes()


# ---- prediction error and merge estimation -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("case", ["merge8_had", "merge8_sad", "merge10_had"])
def test_pred_error_and_merge_estimate(case, geom):
    from nnfme import merge
    from nnfme.runtime import FmeContext
    from test_merge_numpy import load_merge_golden
    g = load_merge_golden(case)
    keep = []
    ctx = FmeContext(device=0, use_hadamard=int(g["use_hadamard"][0]), nn_mode=0, bit_depth=int(g["bit_depth"][0]))
    try:
        _bind_pictures(ctx, keep, g["luma"], geom)
        for lid, lam in enumerate(g["lambdas"]):
            ctx.set_lambda(lid, float(lam))
        dist = merge.pred_error(ctx, g["tasks"])
        assert merge.pred_error_invalid_count(ctx) == 0
        res = merge.merge_estimate(ctx, g["reqs"])   # an invalid request makes it raise
    finally:
        ctx.close()
    bad = np.flatnonzero(dist != g["dist"])
    assert bad.size == 0, (bad[:10], dist[bad[:10]], g["dist"][bad[:10]], g["tasks"][bad[:10]])
    for f in merge.MERGE_RES_DTYPE.names:
        bad = np.flatnonzero((res[f] != g["res"][f]).reshape(len(res), -1).any(axis=1))
        assert bad.size == 0, (f, bad[:10], res[f][bad[:10]], g["res"][f][bad[:10]])


# ---- skip check: luma and chroma ----------------------------------------------------------------------
def _bind_yuv(ctx, keep, ys, cbs, crs, geom):
    for k in range(len(ys)):
        bind_luma(ctx, keep, k, ys[k], geom)
        bind_chroma(ctx, keep, k, cbs[k], crs[k], geom)


def _check_skip(ctx, g):
    from nnfme import skip
    for tasks, want in ((g["tasks"], g["sse"]), (g["req_tasks"], g["req_sse"])):
        got = skip.pred_sse(ctx, tasks)
        assert skip.pred_sse_invalid_count(ctx) == 0
        assert got.shape == want.shape and got.dtype == np.uint32
        for c, comp in enumerate(("Y", "Cb", "Cr")):
            bad = np.flatnonzero(got[:, c] != want[:, c])
            assert bad.size == 0, (comp, bad[:10], got[bad[:10]], want[bad[:10]], tasks[bad[:10]])
    res = np.zeros(len(g["reqs"]), skip.SKIP_RES_DTYPE)
    for s in range(len(g["params"])):   # an invalid request makes it raise
        m = g["req_slice"] == s
        res[m] = skip.skip_estimate(ctx, g["params"][s], g["reqs"][m])
    assert res.tobytes() == g["res"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES_YUV)
@pytest.mark.parametrize("case", ["skip8", "skip10"])
def test_pred_sse_and_skip_estimate(case, geom):
    from nnfme.runtime import FmeContext
    from test_skip_numpy import load_skip_golden
    g = load_skip_golden(case)
    keep = []
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=int(g["bit_depth"][0]))
    try:
        _bind_yuv(ctx, keep, g["y"], g["cb"], g["cr"], geom)
        _check_skip(ctx, g)
    finally:
        ctx.close()


# ---- motion compensation: references and chroma bound, output planes contiguous --------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES_YUV)
@pytest.mark.parametrize("case", ["mc_ra_bi_clip", "mc_ldp_uni", "mc10_ra_bi_clip", "mcwp_b_bi", "mc_shapes"])
def test_motion_compensate(case, geom):
    from nnfme.runtime import FmeContext
    g = load_golden(case)
    fill = int(g["fill"][0]) if "fill" in g else 0
    keep = []
    ctx = FmeContext(nn_mode=0, bit_depth=golden_bit_depth(g))
    try:
        _bind_yuv(ctx, keep, g["ref_y"], g["ref_cb"], g["ref_cr"], geom)
        if "wp" in g:
            for l in range(2):
                for r in range(g["wp"].shape[1]):
                    ctx.set_wp(l, r, g["wp"][l, r])
        got = tuple(np.full_like(g[f], fill) for f in ("pred_y", "pred_cb", "pred_cr"))
        ctx.motion_compensate(g["jobs"], *got)   # an invalid job makes it raise
        assert ctx.mc_invalid_count() == 0
    finally:
        ctx.close()
    for p, f in zip(got, ("pred_y", "pred_cb", "pred_cr")):
        assert np.array_equal(p, g[f]), f"{case} in geometry {geom}, {f}: {int((p != g[f]).sum())} samples differ"


# ---- the producers: bi-pred keys, predInterSearch on P and B slices -----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["A", "C"])
def test_device_bipred_keys_then_refine(geom):
    from test_pred_inter_b import check_device_bipred_keys_drive_refine_like_host_keys
    keep = []
    check_device_bipred_keys_drive_refine_like_host_keys(picture_binder(geom, keep))
    assert len(keep) == 12   # six pictures in each of the two contexts


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["A", "C"])
def test_pred_inter_p(geom):
    from test_pred_inter import check_pred_inter_matches_oracle
    keep = []
    check_pred_inter_matches_oracle(picture_binder(geom, keep))
    assert len(keep) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["A", "C"])
def test_main10_pred_inter_b(geom):
    from test_main10_producers import check_main10_pred_inter_b_matches_oracle
    keep = []
    check_main10_pred_inter_b_matches_oracle(1, picture_binder(geom, keep))
    assert len(keep) == 6


# ---- host planes: row-strided numpy views ------------------------------------------------------------
def host_view(plane, mx, my, stride, seed):
    """plane as a view into a wider, poisoned host array (rows `stride` samples apart)."""
    buf, origin = embed_numpy(plane, mx, my, stride, seed)
    v = plane_view(buf, origin, stride, *plane.shape)
    assert not v.flags.c_contiguous and np.array_equal(v, plane)
    return v


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_strided_views_are_passed_uncopied(dtype):
    """What set_picture / set_picture_chroma hand to the library: the view's own memory and stride; a
    plane that the stride argument cannot describe is copied."""
    from nnfme.runtime import _rows
    plane = np.random.default_rng(2).integers(0, 200, (6, 8), dtype=dtype)
    v = host_view(plane, 3, 1, 13, 4)
    a, stride = _rows(v, dtype)
    assert stride == 13 and a.ctypes.data == v.ctypes.data and a.shape == (6, 8)
    a, stride = _rows(plane, dtype)
    assert stride == 8 and a.ctypes.data == plane.ctypes.data
    for odd in (plane[:, ::2], plane[::-1], plane.astype(np.int32), plane.tolist()):
        a, stride = _rows(odd, dtype)
        assert a.flags.c_contiguous and a.dtype == dtype and stride == a.shape[1] and np.array_equal(a, np.asarray(odd))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["qp32_nn", "main10_fen3_qp27_nn"])
def test_set_picture_from_strided_host_views(case):
    from nnfme.runtime import FmeContext
    from test_gpu_parity import _assert_same
    g = load_golden(case)
    bd = golden_bit_depth(g)
    hadme, fen, nn_mode, qp = (int(v) for v in g["config"])
    ctx = FmeContext(use_hadamard=hadme, nn_mode=nn_mode, qp=qp, fast_inter_mode=fen, bit_depth=bd)
    try:
        for k, p in enumerate(g["pictures"]):
            assert p.dtype == _sample_dtype(bd)
            mx, my, stride = luma_geometry("C", p.shape[1], bd, k)
            ctx.set_picture(k, host_view(p, mx, my, stride, 100 + k))
        for i, lam in enumerate(g["lambdas"]):
            ctx.set_lambda(i, float(lam))
        if g["keys"].size:
            ctx.set_keys(g["keys"])
        res = ctx.refine(g["jobs"])
        assert ctx.refine_status() == 0
    finally:
        ctx.close()
    _assert_same(res, g["results"], case + " from strided host views")


@pytest.mark.gpu
def test_set_picture_chroma_from_strided_host_views():
    from nnfme.runtime import FmeContext
    from test_skip_numpy import load_skip_golden
    g = load_skip_golden("skip8")
    ctx = FmeContext(device=0, use_hadamard=1, nn_mode=0, bit_depth=8)
    try:
        for k in range(len(g["y"])):
            y, cb, cr = g["y"][k], g["cb"][k], g["cr"][k]
            ctx.set_picture(k, host_view(y, *luma_geometry("C", y.shape[1], 8, k), 200 + k))
            mx, my, stride = chroma_geometry("C", cb.shape[1])
            ctx.set_picture_chroma(k, host_view(cb, mx, my, stride, 300 + k), host_view(cr, mx, my, stride, 400 + k))
        _check_skip(ctx, g)
    finally:
        ctx.close()
