"""GPU parity of motion compensation: the HIP path through the C-ABI
(fme_motion_compensate / fme_motion_compensate_device) against the golden planes made by the
reference's own TComInterpolationFilter + TComYuv::addAvg (oracle/_ref) and against the C
restatement (orc_mc) on a full 1080p frame partition.  Integer output: bit-exact."""
import numpy as np
import pytest

from conftest import load_golden, mc10_golden_cases, mc_golden_cases, mc_inputs
from nnfme import synth
from nnfme.abi import MC_JOB_DTYPE, MC_L0, MC_L1

pytestmark = pytest.mark.gpu


def _ctx(pics):
    from nnfme.runtime import FmeContext
    ctx = FmeContext(nn_mode=0)
    for k, (y, cb, cr) in pics.items():
        ctx.set_picture_yuv(k, y, cb, cr)
    return ctx


def _same(got, exp, what):
    for g, e, comp in zip(got, exp, ("Y", "Cb", "Cr")):
        assert np.array_equal(g, e), f"{what} {comp}: {int((g != e).sum())} samples differ"


@pytest.mark.parametrize("case", mc_golden_cases())
def test_mc_golden(case):
    g = load_golden(case)
    pics, jobs, planes = mc_inputs(g)
    _ctx(pics).motion_compensate(jobs, *planes)
    _same(planes, (g["pred_y"], g["pred_cb"], g["pred_cr"]), case)


@pytest.mark.parametrize("case", mc10_golden_cases())
def test_mc10_golden(case):
    """Bit depth 10 (main10): uint16 planes through fme_motion_compensate against the reference's
    own filters and addAvg at bitDepth 10 (k_mc<true>)."""
    from nnfme.runtime import FmeContext
    g = load_golden(case)
    pics, jobs, planes = mc_inputs(g)
    ctx = FmeContext(nn_mode=0, bit_depth=10)
    for k, (y, cb, cr) in pics.items():
        ctx.set_picture_yuv(k, y, cb, cr)
    ctx.motion_compensate(jobs, *planes)
    _same(planes, (g["pred_y"], g["pred_cb"], g["pred_cr"]), case)


def test_mc10_device_frame_matches_reference():
    """A 416x240 main10 partition (every PU shape, 40 % bi-pred, MVs up to +-150 quarter-pel so
    clipMv acts at the borders) with device-resident jobs and uint16 planes, against oracle/_ref
    at bitDepth 10 run live."""
    import torch
    from nnfme.runtime import FmeContext
    from oracle import Reference
    W, H = 416, 240
    rng = np.random.default_rng(5)
    pics = {}
    for k in range(3):
        cb, cr = synth.synth_chroma(W, H, k)
        lo = rng.integers(0, 4, size=(2,) + cb.shape, dtype=np.uint16)
        pics[k] = (synth.synth_luma_hbd(W, H, k, bit_depth=10), (cb.astype(np.uint16) << 2) | lo[0],
                   (cr.astype(np.uint16) << 2) | lo[1])
    jobs = synth.make_mc_partition(rng, W, H, [0, 1, 2], bi_frac=0.4, mv_amp=150, identical_frac=0.1)
    ctx = FmeContext(nn_mode=0, bit_depth=10)
    ref = Reference(bit_depth=10)
    for k, p in pics.items():
        ctx.set_picture_yuv(k, *p)
        ref.set_picture_yuv(k, *p)
    dev = torch.device("cuda", 0)
    dj = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    dy = torch.zeros((H, W), dtype=torch.int16, device=dev)
    dcb = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
    dcr = torch.zeros_like(dcb)
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.motion_compensate_device(dj.data_ptr(), len(jobs), dy.data_ptr(), W, dcb.data_ptr(), dcr.data_ptr(), W // 2,
                                 W, H, s)
    assert ctx.mc_invalid_count() == 0
    exp = (np.zeros((H, W), np.uint16), np.zeros((H // 2, W // 2), np.uint16), np.zeros((H // 2, W // 2), np.uint16))
    ref.mc(jobs, *exp)
    got = tuple(t.cpu().numpy().view(np.uint16) for t in (dy, dcb, dcr))
    _same(got, exp, "416x240 main10")


def _frame(W, H, refs, seed):
    pics = {}
    for k in range(refs):
        cb, cr = synth.synth_chroma(W, H, k)
        pics[k] = (synth.synth_luma(W, H, k), cb, cr)
    return pics


def test_mc_device_1080p_matches_oracle():
    """A whole 1080p partition (every PU shape, 30 % bi-pred, 10 % identical motion, MVs up to
    +-96 pel so clipMv acts at the borders), device-resident jobs and planes."""
    import torch
    from oracle import Oracle
    W, H = 1920, 1080
    pics = _frame(W, H, 4, 2)
    rng = np.random.default_rng(77)
    jobs = synth.make_mc_partition(rng, W, H, [0, 1, 2, 3], bi_frac=0.3, mv_amp=96, identical_frac=0.1)
    ctx = _ctx(pics)
    dev = torch.device("cuda", 0)
    dj = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    dy = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    dcb = torch.zeros((H // 2, W // 2), dtype=torch.uint8, device=dev)
    dcr = torch.zeros_like(dcb)
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.motion_compensate_device(dj.data_ptr(), len(jobs), dy.data_ptr(), W, dcb.data_ptr(), dcr.data_ptr(), W // 2,
                                 W, H, s)
    assert ctx.mc_invalid_count() == 0
    exp = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    Oracle().mc(pics, jobs, *exp)
    _same((dy.cpu().numpy(), dcb.cpu().numpy(), dcr.cpu().numpy()), exp, "1080p")
    # run-to-run determinism on the same buffers
    ctx.motion_compensate_device(dj.data_ptr(), len(jobs), dy.data_ptr(), W, dcb.data_ptr(), dcr.data_ptr(), W // 2,
                                 W, H, s)
    _same((dy.cpu().numpy(), dcb.cpu().numpy(), dcr.cpu().numpy()), exp, "1080p rerun")


_SENTINEL = 0xA5   # pre-filled into the output planes: a sample no job owns must keep it


def _small_frame(bit_depth):
    """A 72x40 picture (not a multiple of the CTU) with three references, its partition (half
    bi-pred, a fifth of those with identical motion, MVs up to +-200 pel so clipMv and the edge
    replication act) and the oracle's planes for the first n jobs."""
    from oracle import Oracle
    W, H = 72, 40
    rng = np.random.default_rng(91)
    pics = {}
    for k in range(3):
        cb, cr = synth.synth_chroma(W, H, k)
        if bit_depth == 8:
            pics[k] = (synth.synth_luma(W, H, k), cb, cr)
        else:
            lo = rng.integers(0, 4, size=(2,) + cb.shape, dtype=np.uint16)
            pics[k] = (synth.synth_luma_hbd(W, H, k, bit_depth=10), (cb.astype(np.uint16) << 2) | lo[0],
                       (cr.astype(np.uint16) << 2) | lo[1])
    jobs = synth.make_mc_partition(rng, W, H, [0, 1, 2], bi_frac=0.5, mv_amp=200, identical_frac=0.2)
    dt = np.uint16 if bit_depth > 8 else np.uint8
    orc = Oracle(bit_depth=bit_depth)

    def expect(n):
        exp = tuple(np.full(s, _SENTINEL, dt) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
        orc.mc(pics, jobs[:n], *exp)
        return exp

    return W, H, pics, jobs, expect


_small_frames = {}


def _small(bit_depth):
    if bit_depth not in _small_frames:
        _small_frames[bit_depth] = _small_frame(bit_depth)
    return _small_frames[bit_depth]


def _mc_device(ctx, jobs, W, H, y_stride, c_stride, tdt):
    """Device-resident jobs into sentinel-filled planes of the given strides; returns the planes."""
    import torch
    dev = torch.device("cuda", 0)
    dj = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    dy = torch.full((H, y_stride), _SENTINEL, dtype=tdt, device=dev)
    dcb = torch.full((H // 2, c_stride), _SENTINEL, dtype=tdt, device=dev)
    dcr = torch.full((H // 2, c_stride), _SENTINEL, dtype=tdt, device=dev)
    ctx.motion_compensate_device(dj.data_ptr(), len(jobs), dy.data_ptr(), y_stride, dcb.data_ptr(), dcr.data_ptr(),
                                 c_stride, W, H, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return dy.cpu().numpy(), dcb.cpu().numpy(), dcr.cpu().numpy()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_mc_workgroup_boundaries(bit_depth, n):
    """k_mc's workgroup tiling (kMcJobs = 8 jobs per workgroup): one job, a part group, exactly one
    group, one over, two groups plus one.  Every sample equals the oracle's on the same n jobs, so
    every sample outside the n PUs still holds the sentinel; no job is rejected."""
    import torch
    from nnfme.runtime import FmeContext
    W, H, pics, jobs, expect = _small(bit_depth)
    assert len(jobs) >= 17
    ctx = FmeContext(nn_mode=0, bit_depth=bit_depth)
    for k, p in pics.items():
        ctx.set_picture_yuv(k, *p)
    tdt, ndt = (torch.uint8, np.uint8) if bit_depth == 8 else (torch.int16, np.uint16)
    got = tuple(p.view(ndt) for p in _mc_device(ctx, jobs[:n], W, H, W, W // 2, tdt))
    assert ctx.mc_invalid_count() == 0
    exp = expect(n)
    _same(got, exp, f"{bit_depth}-bit, {n} jobs")
    own = np.zeros((H, W), bool)
    for j in jobs[:n]:
        own[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]] = True
    assert (got[0][~own] == _SENTINEL).all()
    assert (got[1][~own[::2, ::2]] == _SENTINEL).all() and (got[2][~own[::2, ::2]] == _SENTINEL).all()


def test_mc_unaligned_output_planes():
    """8 bits, device form, output strides W + 2 (luma, no multiple of 4) and W/2 + 1 (chroma, odd):
    store_row takes its per-byte path.  The W x H views equal the oracle's contiguous planes and the
    padding columns keep the sentinel."""
    import torch
    W, H, pics, jobs, expect = _small(8)
    ctx = _ctx(pics)
    got = _mc_device(ctx, jobs, W, H, W + 2, W // 2 + 1, torch.uint8)
    assert ctx.mc_invalid_count() == 0
    exp = expect(len(jobs))
    _same((got[0][:, :W], got[1][:, :W // 2], got[2][:, :W // 2]), exp, "unaligned planes")
    for p, w in zip(got, (W, W // 2, W // 2)):
        assert (p[:, w:] == _SENTINEL).all()


def test_mc10_unaligned_output_planes():
    """Bit depth 10, device form, int16 output planes with odd strides W + 1 (luma) and W/2 + 1
    (chroma): every other row starts 2 bytes off a dword, where k_mc<true>'s store_row writes one
    16-bit sample at a time.  The W x H views equal the oracle's contiguous planes and the padding
    column keeps the sentinel."""
    import torch
    from nnfme.runtime import FmeContext
    W, H, pics, jobs, expect = _small(10)
    ctx = FmeContext(nn_mode=0, bit_depth=10)
    for k, p in pics.items():
        ctx.set_picture_yuv(k, *p)
    got = tuple(p.view(np.uint16) for p in _mc_device(ctx, jobs, W, H, W + 1, W // 2 + 1, torch.int16))
    assert ctx.mc_invalid_count() == 0
    exp = expect(len(jobs))
    _same((got[0][:, :W], got[1][:, :W // 2], got[2][:, :W // 2]), exp, "unaligned 10-bit planes")
    for p, w in zip(got, (W, W // 2, W // 2)):
        assert (p[:, w:] == _SENTINEL).all()


def test_mc_invalid_jobs():
    from nnfme.runtime import FmeError
    W, H = 128, 64
    pics = _frame(W, H, 2, 5)
    ctx = _ctx(pics)
    jobs = np.zeros(3, MC_JOB_DTYPE)
    jobs["w"], jobs["h"], jobs["flags"] = 16, 16, MC_L0
    jobs["x"] = [0, 16, 32]
    planes = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    bad = jobs.copy()
    bad["w"][1] = 6                       # not a PU size
    with pytest.raises(FmeError, match="job 1: PU size"):
        ctx.motion_compensate(bad, *planes)
    bad = jobs.copy()
    bad["ref_id"][2, 0] = 7               # no such picture
    with pytest.raises(FmeError, match="job 2"):
        ctx.motion_compensate(bad, *planes)
    bad = jobs.copy()
    bad["flags"][0] = 0                   # no list
    with pytest.raises(FmeError, match="job 0"):
        ctx.motion_compensate(bad, *planes)
    assert not planes[0].any()            # nothing ran
    ctx.set_picture(5, synth.synth_luma(W, H, 3))   # luma only: no motion compensation from it
    bad = jobs.copy()
    bad["flags"][0] = MC_L0 | MC_L1
    bad["ref_id"][0] = (0, 5)
    with pytest.raises(FmeError, match="chroma"):
        ctx.motion_compensate(bad, *planes)
    # device path: invalid jobs are skipped and counted, the rest still predicted
    import torch
    from oracle import Oracle
    dev = torch.device("cuda", 0)
    bad = jobs.copy()
    bad["x"][1] = W - 8                   # outside the picture
    dj = torch.from_numpy(bad.view(np.uint8).copy()).to(dev)
    dy = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    dcb = torch.zeros((H // 2, W // 2), dtype=torch.uint8, device=dev)
    dcr = torch.zeros_like(dcb)
    ctx.motion_compensate_device(dj.data_ptr(), 3, dy.data_ptr(), W, dcb.data_ptr(), dcr.data_ptr(), W // 2, W, H,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert ctx.mc_invalid_count() == 1
    exp = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    Oracle().mc({0: pics[0]}, bad[[0, 2]], *exp)
    _same((dy.cpu().numpy(), dcb.cpu().numpy(), dcr.cpu().numpy()), exp, "skip invalid")


def test_mc_empty_and_profiled():
    W, H = 64, 64
    pics = _frame(W, H, 1, 9)
    ctx = _ctx(pics)
    planes = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    ctx.motion_compensate(np.zeros(0, MC_JOB_DTYPE), *planes)
    ctx.set_profiling(True)
    jobs = synth.make_mc_partition(np.random.default_rng(1), W, H, [0])
    ctx.motion_compensate(jobs, *planes)
    assert ctx.mc_last_ms() > 0.0
