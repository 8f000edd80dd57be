"""The lane search kernels' wave tiles and record stores at their edges, at bit depths 8 and 10
(csrc/fme_lane.hip, csrc/fme_lane10.hip over csrc/fme_lane_common.h): tiles with one live PU and the
rest inactive, full tiles followed by a partial one, the two-units-per-lane classes, the padded AMP
groups and keyed jobs, every field of every record against oracle/_ref run live."""
import numpy as np
import pytest

from nnfme import synth, weights
from nnfme.abi import compare_results

pytestmark = pytest.mark.gpu

W, H = 416, 240
FIELDS = ("mv_int_x", "mv_int_y", "half_x", "half_y", "qtr_x", "qtr_y", "frac_cost", "c", "n_emi",
          "nn_class", "mv_x", "mv_y", "bits", "cost")


def _batch(rng, per_class):
    """per_class jobs of each of the 24 PU shapes, the shapes interleaved in call order."""
    assert len(synth.ALL_PU_SIZES) == 24
    w = np.tile(np.array([s[0] for s in synth.ALL_PU_SIZES]), per_class)
    h = np.tile(np.array([s[1] for s in synth.ALL_PU_SIZES]), per_class)
    return synth.make_jobs(rng, W, H, len(w), 4, [0, 1, 2, 3], [0, 1, 2, 3], sizes=(w, h), bipred_frac=0.2)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_lane_tiles_every_record_against_reference(bit_depth):
    """Batch A: one job per class (every class's only tile holds one live PU).  Batch B: 65 jobs per
    class (1,560 jobs: at least one full tile and a partial one for every class, 64 PUs per tile for
    the one-lane 4x8 shape down to one for 64x64).  Each from a fresh NN state."""
    from oracle import Reference
    from nnfme.runtime import FmeContext
    times = (7, 6, 5, 4, 0)
    if bit_depth == 8:
        pics = {k: synth.synth_luma(W, H, t) for k, t in zip(range(5), times)}
    else:
        pics = {k: synth.synth_luma_hbd(W, H, t, bit_depth) for k, t in zip(range(5), times)}
    ctx = FmeContext(nn_mode=1, qp=22, fast_inter_mode=1, max_jobs=65 * 24, bit_depth=bit_depth)
    ref = Reference(use_hadamard=1, nn_mode=1, fast_inter_mode=1, bit_depth=bit_depth)
    for e in (ctx, ref):
        for k, v in pics.items():
            e.set_picture(k, v)
        for lid, lam in enumerate(synth.LDP_LAMBDA[22]):
            e.set_lambda(lid, lam)
    ref.load_nn(weights.load_weights(22))
    rng = np.random.default_rng(900 + bit_depth)
    for name, per_class in (("A", 1), ("B", 65)):
        jobs = _batch(rng, per_class)
        keys = synth.make_bipred_keys(rng, jobs, pics)
        assert len(jobs) == 24 * per_class and (per_class == 1 or len(keys) > 0)
        for e in (ctx, ref):
            if len(keys):
                e.set_keys(keys)
            e.nn_reset()
        got = ctx.refine(jobs)
        want = ref.refine(jobs)
        bad, first, counts = compare_results(got, want, FIELDS)
        assert bad == 0, f"batch {name}, {bit_depth} bits: {bad} of {len(jobs)} jobs differ, first {first}: {counts}"
