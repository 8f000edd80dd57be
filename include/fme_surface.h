/* fme_surface.h — the sub-pel cost surface of a PU: the cost of all 49 quarter-pel positions within
 * +-3/4 pel of an integer MV, on the GPU.
 *
 * Additional exports of libfme_amd.so beside include/fme.h (they are not part of the
 * FME_ABI_VERSION-counted set).  xPatternSearchFracDIF (TEncSearch.cpp:4804-4855) visits 17 of these
 * positions in two stages; NN_pred() names one of them as its class.  This entry point returns what
 * every one of them costs, in the search's own terms, so that a caller can price the NN's pick, the
 * search's pick and the true minimum against each other.  Per job and position (dx, dy), each in
 * -3..3, i.e. the quarter-pel MV (4 mv_x + dx, 4 mv_y + dy):
 *   prediction   normative xPredInterBlk luma (TComPrediction.cpp:596-668): the two-stage 8-tap filter
 *                with 14-bit intermediates, uni-pred, clipped to the bit depth; no clipMv, picture
 *                edges replicated: what xExtDIFUpSamplingH / Q yield at every candidate;
 *   dist         FracDIF's setDistParam variant (TComRdCost.cpp:233-275): with HADME on and the job
 *                not lossless xGetHADs (8x8 tiles when w and h are multiples of 8, else 4x4),
 *                otherwise the SAD; the PU's sum shifted right by bitDepth - 8 once; against the
 *                original at (x, y), or the int16 key block at key_offset (fme_set_keys);
 *   cost         dist + getCostOfVectorWithPredictor at cost scale 0 with the motion lambda of
 *                lambda_id and the job's mvp: (UInt)(mlambda * bits / 65536.0), UInt arithmetic
 *                (wrap-around included).
 * The surface is centred on the job's full-pel (mv_x, mv_y) exactly as given: no EMI step runs, and
 * FME_JOB_EMI, FME_JOB_NN_IN, lt_* / rb_* and bits_in are ignored.  A caller who wants the surface a
 * refinement saw passes mv := fme_result.mv_int.  NN state, pictures and tables are only read.   */
#ifndef FME_SURFACE_H_
#define FME_SURFACE_H_

#include "fme.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_SURF_POINTS 49
/* index of quarter-pel offset (dx, dy), each in -3..3, around the integer MV: equals the NN_pred
 * class of that offset */
#define FME_SURF_INDEX(dx, dy) (((dy) + 3) * 7 + (dx) + 3)
#define FME_SURF_NO_PROBE 0xFFu

typedef struct fme_surface {
  uint32_t dist[FME_SURF_POINTS];
  uint32_t cost[FME_SURF_POINTS];
} fme_surface;   /* 392 bytes */

typedef struct fme_surface_pick {
  uint32_t min_cost;        /* least cost[]; the first index wins a tie (strict <, index order 0..48) */
  uint32_t probe_cost[2];   /* cost[probe[k]], 0xFFFFFFFF for FME_SURF_NO_PROBE                        */
  uint8_t  min_idx, probe[2], status;   /* status 0, or 1 = invalid job (device form)                  */
} fme_surface_pick;   /* 16 bytes */

/* One fme_job per surface.  probe (two position indices per job, 0..48 or FME_SURF_NO_PROBE) may be
 * null: every probe is then FME_SURF_NO_PROBE.  surf and pick may each be null, not both.
 * A job is valid as in a refine batch: one of the 24 PU shapes, the reference slot set, lambda_id
 * below FME_MAX_LAMBDAS, and either the key block inside the key buffer (key_offset >= 0) or the
 * original slot set, of the reference's size, with the PU inside it; a probe is 0..48 or
 * FME_SURF_NO_PROBE.
 * fme_cost_surface: host arrays, synchronous; a batch with any invalid job is rejected
 *   (FME_E_INVALID, nothing runs, nothing is written); n == 0 returns 0.
 * fme_cost_surface_device: device arrays, stream-ordered, no host synchronisation; an invalid job
 *   gets 0xFFFFFFFF in every word of its surface and pick costs and status 1, and is counted;
 *   fme_cost_surface_invalid_count() waits and returns the count of the last such call.         */
int fme_cost_surface(fme_ctx* ctx, const fme_job* jobs, const uint8_t (*probe)[2], fme_surface* surf,
                     fme_surface_pick* pick, int n, void* stream);
int fme_cost_surface_device(fme_ctx* ctx, const fme_job* d_jobs, const uint8_t (*d_probe)[2], fme_surface* d_surf,
                            fme_surface_pick* d_pick, int n, void* stream);
int fme_cost_surface_invalid_count(fme_ctx* ctx);
/* With profiling on: device milliseconds of the last surface launch; waits for it. */
int fme_cost_surface_last_ms(fme_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* FME_SURFACE_H_ */
