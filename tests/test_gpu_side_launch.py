"""What the side launches share (csrc/fme_ctx.h: LaunchTimer, InvalidCounter): motion compensation,
prediction error, SSE, cost surface and integer search each time their one launch the same way, and
the three fused prediction kernels count the tasks they skip the same way.  This pins the states of
*_last_ms (no profiled launch / a time / none again once a launch went out unprofiled) and of
*_invalid_count (0 before any launch / the skipped tasks of the last device-form launch, read behind
the stream it went out on / 0 after a clean one), at both bit depths.

One 64x64 picture pair with chroma and four PUs of 8x4, 4x8, 8x8 and 16x16: the smallest shapes that
reach every lane-group size class of the prediction kernels."""
import numpy as np
import pytest

from nnfme import merge, skip, surface, synth
from nnfme.abi import E_STATE, JOB_DTYPE, JOB_EMI, MC_JOB_DTYPE, MC_L0, TZ_EXT_DTYPE
from nnfme.runtime import FmeContext, FmeError

pytestmark = pytest.mark.gpu

W = H = 64
SHAPES = ((8, 4), (4, 8), (8, 8), (16, 16))
AT = ((8, 8), (24, 8), (8, 24), (32, 32))   # each PU at the origin of its CU, 8 samples inside the picture
UNSET = 9                                   # a picture slot nothing is bound to
RANGE = 8                                   # integer search range, in samples: the windows stay inside the picture


def make_ctx(bit_depth, **kw):
    """Pictures 0 (the original) and 1 (the reference) with chroma, lambda 0."""
    ctx = FmeContext(nn_mode=0, bit_depth=bit_depth, **kw)
    for k in range(2):
        cb, cr = synth.synth_chroma(W, H, k)
        if bit_depth == 8:
            ctx.set_picture_yuv(k, synth.synth_luma(W, H, k), cb, cr)
        else:
            ctx.set_picture_yuv(k, synth.synth_luma_hbd(W, H, k, bit_depth), cb.astype(np.uint16) << 2,
                                cr.astype(np.uint16) << 2)
    ctx.set_lambda(0, synth.LDP_LAMBDA[22][1])
    return ctx


def _place(a):
    for i, ((w, h), (x, y)) in enumerate(zip(SHAPES, AT)):
        a["x"][i], a["y"][i], a["w"][i], a["h"][i] = x, y, w, h
    return a


def pred_tasks(dtype):
    """The four PUs as fme_pe_task / fme_sse_task / fme_mc_job rows: list 0, reference 1, a quarter-pel MV."""
    t = _place(np.zeros(len(SHAPES), dtype))
    t["cu_x"], t["cu_y"] = t["x"], t["y"]
    t["flags"] = MC_L0
    t["ref_id"][:, 0] = 1
    t["mv"][:, 0] = (5, -3)
    return t


def search_jobs():
    """The four PUs as fme_job rows (cost surface, integer search, refinement) and their fme_tz_ext."""
    j = _place(np.zeros(len(SHAPES), JOB_DTYPE))
    j["ref_id"], j["flags"], j["bits_in"], j["key_offset"] = 1, JOB_EMI, 1, -1
    j["lt_x"] = j["lt_y"] = -RANGE
    j["rb_x"] = j["rb_y"] = RANGE
    ext = np.zeros(len(j), TZ_EXT_DTYPE)
    ext["cu_x"], ext["cu_y"], ext["search_range"] = j["x"], j["y"], RANGE
    return j, ext


def mc_planes(bit_depth):
    dt = np.uint8 if bit_depth == 8 else np.uint16
    return np.zeros((H, W), dt), np.zeros((H // 2, W // 2), dt), np.zeros((H // 2, W // 2), dt)


# family -> (one host-form call, *_last_ms, the text behind "no profiled ")
FAMILIES = {
    "mc": (lambda c: c.motion_compensate(pred_tasks(MC_JOB_DTYPE), *mc_planes(c.bit_depth)),
           lambda c: c.mc_last_ms(), "fme_mc_last_ms: no profiled motion compensation"),
    "pred_error": (lambda c: merge.pred_error(c, pred_tasks(merge.PE_TASK_DTYPE)),
                   lambda c: merge.pred_error_last_ms(c), "fme_pred_error_last_ms: no profiled prediction-error launch"),
    "pred_sse": (lambda c: skip.pred_sse(c, pred_tasks(skip.SSE_TASK_DTYPE)),
                 lambda c: skip.pred_sse_last_ms(c), "fme_pred_sse_last_ms: no profiled SSE launch"),
    "surface": (lambda c: surface.cost_surface(c, search_jobs()[0]),
                lambda c: surface.cost_surface_last_ms(c), "fme_cost_surface_last_ms: no profiled surface launch"),
    "integer_search": (lambda c: c.integer_search(*search_jobs()),
                       lambda c: c.integer_search_last_ms(), "fme_integer_search_last_ms: no profiled integer search"),
}


@pytest.mark.parametrize("bit_depth", [8, 10])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_last_ms_follows_the_last_launch(family, bit_depth):
    call, last_ms, text = FAMILIES[family]
    ctx = make_ctx(bit_depth)
    try:
        def refused():
            with pytest.raises(FmeError) as e:
                last_ms(ctx)
            assert e.value.code == E_STATE and str(e.value).endswith(text), str(e.value)
        refused()                 # nothing launched
        call(ctx)
        refused()                 # launched with profiling off
        ctx.set_profiling(True)
        call(ctx)
        assert last_ms(ctx) > 0
        ctx.set_profiling(False)
        call(ctx)
        refused()                 # `timed` is the last launch's
    finally:
        ctx.close()


def _two_invalid(rows):
    """A size of 6 and an unset reference picture: what each kernel's validator rejects."""
    bad = rows.copy()
    bad["w"][0] = 6
    if bad["ref_id"].ndim == 2:
        bad["ref_id"][2, 0] = UNSET
    else:
        bad["ref_id"][2] = UNSET
    return bad


def _counted(family):
    """(rows, device-form launch of n rows on a stream, *_invalid_count) of a counting family."""
    import torch
    if family == "pred_error":
        out = torch.zeros(len(SHAPES), dtype=torch.int32, device="cuda")
        return (pred_tasks(merge.PE_TASK_DTYPE), lambda c, d, s: merge.pred_error_device(c, d, out, len(SHAPES), s),
                merge.pred_error_invalid_count)
    if family == "pred_sse":
        out = torch.zeros(3 * len(SHAPES), dtype=torch.int32, device="cuda")
        return (pred_tasks(skip.SSE_TASK_DTYPE), lambda c, d, s: skip.pred_sse_device(c, d, out, len(SHAPES), s),
                skip.pred_sse_invalid_count)
    out = torch.zeros(98 * len(SHAPES), dtype=torch.int32, device="cuda")
    return (search_jobs()[0], lambda c, d, s: surface.cost_surface_device(c, d, None, out, None, len(SHAPES), s),
            surface.cost_surface_invalid_count)


@pytest.mark.parametrize("bit_depth", [8, 10])
@pytest.mark.parametrize("family", ["pred_error", "pred_sse", "surface"])
def test_invalid_count_is_the_last_launch_s(family, bit_depth):
    import torch
    rows, launch, count = _counted(family)
    d_good = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_bad = torch.from_numpy(_two_invalid(rows).view(np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()      # the uploads went out on the default stream
    ctx = make_ctx(bit_depth)
    try:
        assert count(ctx) == 0    # before any launch
        launch(ctx, d_bad, side.cuda_stream)
        assert count(ctx) == 2    # waits for the side stream, nothing else synchronises here
        launch(ctx, d_good, side.cuda_stream)
        assert count(ctx) == 0
    finally:
        ctx.close()
