/* fme_direct.h — NN-direct refinement: the EMI step, NN_pred(), and one sub-pel evaluation at the
 * net's own position instead of xPatternSearchFracDIF's 17.
 *
 * Additional exports of libfme_amd.so beside include/fme.h (they are not part of the
 * FME_ABI_VERSION-counted set).  The shipped encoder (TEncSearch.cpp:4534-4597) runs FracDIF in
 * full, lets NN_pred() overwrite the MV, and keeps FracDIF's ruiCost: the cost of an MV it does not
 * return.  fme_refine* reproduce that bit for bit.  The entry points here run the mode the net was
 * trained for: per job the EMI square step, the net, one prediction at the net's class, and
 * xMotionEstimation's tail on that position's cost.  The results therefore differ from the shipped
 * encoder's by design: frac_cost / cost are those of the returned MV.
 *
 * Contexts: nn_mode 1 (weights loaded) and nn_mode 2 (net loaded), either engine, bit depth 8 and
 * 10; nn_mode 0 returns FME_E_STATE (there is no class to evaluate).  A job is valid as in fme_refine.
 *
 * The record of a job, against what fme_refine gives for the same job stream and incoming NN state:
 *   mv_int_*, c, emi[], n_emi, nn_class, FME_RES_NN_STALE / FME_RES_NN_UNINIT   identical (jobs
 *               without FME_JOB_EMI, FME_JOB_NN_IN rows and FME_NN_IN_SLOT_RESET nets included), and
 *               so is the NN state carried out of the batch: direct and ordinary batches advance the
 *               same context state and may be interleaved;
 *   half_*, qtr_*  the four globals of the class as fme_nn_pred_single returns them in out4 (the
 *               switch at TEncSearch.cpp:136-193): not a search result;
 *   mv_*        4 mv_int + (cls % 7 - 3, cls / 7 - 3), as fme_refine;
 *   frac_cost   the cost of that position in fme_surface.h's terms, fme_surface.cost[nn_class] of
 *               the surface centred on mv_int: normative two-stage luma prediction (no clipMv, edges
 *               replicated), FracDIF's distortion (xGetHADs 8x8 / 4x4, or the SAD when HADME is off
 *               or the job is lossless; the PU's sum >> bitDepth - 8 once) against the original or the
 *               int16 key block, plus getCostOfVectorWithPredictor at cost scale 0, UInt arithmetic;
 *   bits, cost  fme_refine's tail fed with that frac_cost:
 *               floor(fW (frac_cost - getCost(mvBits))) + getCost(bits), fW 0.5 for FME_JOB_BIPRED;
 *   status      fme_refine's bits | FME_RES_NN_DIRECT.
 *
 * Ordering: a direct batch starts after every refinement batch issued before it has finished and
 * every later batch of either kind starts after it; it takes no part in the overlap of consecutive
 * ordinary batches.  fme_refine_status, fme_nn_get_state, fme_nn_copy_state_device and a following
 * batch behave as after an ordinary batch.                                                        */
#ifndef FME_DIRECT_H_
#define FME_DIRECT_H_

#include "fme.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_RES_NN_DIRECT 0x04u   /* frac_cost / cost are those of the NN's own position */

/* Host arrays, synchronous, as fme_refine: a batch that holds an invalid job returns FME_E_INVALID
 * (nothing computed, the NN state unchanged); n == 0 returns 0. */
int fme_refine_direct(fme_ctx* ctx, const fme_job* jobs, fme_result* res, int n, void* stream);
/* Device arrays, stream-ordered, no host synchronisation, fme_refine_device's contract: validated
 * on the device; in a rejected batch every record gets FME_RES_REJECTED, the NN state is carried
 * through unchanged and fme_refine_status() returns the count. */
int fme_refine_direct_device(fme_ctx* ctx, const fme_job* d_jobs, fme_result* d_res, int n, void* stream);
/* The same with the 16-byte records of fme_refine_mv_device. */
int fme_refine_direct_mv_device(fme_ctx* ctx, const fme_job* d_jobs, fme_mv_result* d_out, int n, void* stream);
/* With profiling on: device milliseconds of the last direct batch (waits for it): the EMI kernel,
 * the class kernel, the evaluation kernel, the whole batch (front end included). */
int fme_refine_direct_last_ms(fme_ctx* ctx, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* FME_DIRECT_H_ */
