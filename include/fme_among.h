/* fme_among.h — candidate-set refinement: the best of up to 8 sub-pel positions per job, the shipped
 * net's K highest outputs as such a list, and the two chained.
 *
 * Additional exports of libfme_amd.so beside include/fme.h (they are not part of the
 * FME_ABI_VERSION-counted set).  fme_refine_at* (include/fme_extern.h) evaluates one class per job;
 * a direct batch (include/fme_direct.h) the net's argmax.  The families here are the middle between
 * one position and the whole search: fme_refine_among* takes a list of k candidate classes per job
 * and keeps the one of least cost, the job set-up, the reference window and the target shared by the
 * candidates; fme_nn_rank_device turns rows of NN inputs into the k classes the loaded two-layer net
 * rates highest; fme_refine_topk* is fme_nn_inputs_device, the ranking and the among evaluation in
 * one batch.
 *
 * fme_refine_among*: cand holds n*k bytes, job i's slots at cand[i*k .. i*k+k-1].  A slot is a class
 *   0..48 or FME_AMONG_EMPTY (skipped); duplicates are allowed.  Each non-empty slot s has
 *   frac_cost_s = fme_surface.cost[cand[i][s]] of the surface centred on mv_int.  The chosen slot is
 *   the one of least frac_cost_s, the earliest on equal cost (strict <, in slot order).  The record:
 *   nn_class, half_*, qtr_*, mv_*, frac_cost, bits, cost   fme_refine_at's for the chosen class;
 *   mv_int_*, c, emi[], n_emi   as in fme_refine_at: from the row when rows are given, else the EMI
 *               step runs;
 *   status      FME_RES_NN_DIRECT | FME_RES_NN_EXTERN | FME_RES_NN_AMONG.
 *   cand_cost (may be NULL; n*k words): cand_cost[i*k+s] = frac_cost_s; 0xFFFFFFFF for an empty slot
 *   and for every slot of a refused job or a rejected batch.
 *   The NN state is neither read nor written, and a pending set / reset stays pending.
 *   Jobs refused one by one: a slot value in 49..254, a list whose slots are all empty, or a row that
 *   fme_refine_at would refuse (marked FME_RES_REJECTED, or its integer MV more than one sample from
 *   the job's mv).  Such a job's record is 0 but for status = FME_RES_REJECTED, the other jobs are
 *   unaffected, and fme_refine_among_status() counts them.  An invalid job rejects the whole batch
 *   as in fme_refine_device (fme_refine_status()).
 *   k outside 1..FME_AMONG_MAX: FME_E_INVALID.  Bound NN input rows (fme_set_nn_inputs): FME_E_STATE.
 *   Every nn_mode, 8 and 10 bits.
 *
 * fme_nn_rank_device: per fme_nn_row the k classes with the highest outputs of the loaded two-layer
 *   net, slot 0 the highest, equal outputs the lower class first: the first-maximum rule of the NN
 *   tail (strict >, rows in order) applied k times.  The arithmetic is the tail's operation for
 *   operation (float32, every dot product in k order, separate multiply and add, the same
 *   normalisation and embedding prefix), so cand[i][0] is the nn_class fme_refine / fme_refine_direct
 *   records for the same inputs.  A row marked FME_RES_REJECTED gets FME_AMONG_EMPTY in all k slots.
 *   d_cand holds n*k bytes; nothing beyond them is read or written.  Needs nn_mode 1 with weights
 *   loaded: nn_mode 0 returns FME_E_STATE, nn_mode 2 FME_E_UNSUPPORTED.  It reads no NN state.
 *
 * fme_refine_topk*: fme_nn_inputs_device into context-owned rows, fme_nn_rank_device, and the among
 *   evaluation with those rows, as one batch.  The candidates go into the caller's d_cand when given
 *   (it is left filled), else into a context-owned buffer.  The carried NN state is advanced exactly
 *   as by fme_refine_direct over the same jobs, so top-K, direct and ordinary batches interleave.
 *   status: the row's FME_RES_NN_STALE / _UNINIT bits plus FME_RES_NN_DIRECT | FME_RES_NN_AMONG (no
 *   EXTERN bit: the classes are the net's).  With k = 1 the records are fme_refine_direct's apart
 *   from the AMONG bit.  Needs nn_mode 1 (as fme_nn_rank_device).
 *
 * Ordering: all are planned like a direct batch: behind every refinement batch in flight, and every
 * later batch behind them.                                                                        */
#ifndef FME_AMONG_H_
#define FME_AMONG_H_

#include "fme.h"
#include "fme_direct.h"
#include "fme_extern.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_AMONG_MAX   8        /* candidates per job */
#define FME_AMONG_EMPTY 0xFFu    /* an unused slot */
#define FME_RES_NN_AMONG 0x10u   /* the record is the best of a candidate list */

/* Host arrays, synchronous.  The lists (and, with rows, the rows' MVs) are checked before anything
 * is enqueued: FME_E_INVALID, res untouched. */
int fme_refine_among(fme_ctx* ctx, const fme_job* jobs, const fme_nn_row* rows /* may be NULL */,
                     const uint8_t* cand, int k, fme_result* res, uint32_t* cand_cost /* may be NULL */, int n,
                     void* stream);
/* Device arrays, stream-ordered, no host synchronisation. */
int fme_refine_among_device(fme_ctx* ctx, const fme_job* d_jobs, const fme_nn_row* d_rows /* may be NULL */,
                            const uint8_t* d_cand, int k, fme_result* d_res, uint32_t* d_cand_cost /* may be NULL */,
                            int n, void* stream);
/* The same with the 16-byte records of fme_refine_mv_device. */
int fme_refine_among_mv_device(fme_ctx* ctx, const fme_job* d_jobs, const fme_nn_row* d_rows /* may be NULL */,
                               const uint8_t* d_cand, int k, fme_mv_result* d_out,
                               uint32_t* d_cand_cost /* may be NULL */, int n, void* stream);
/* Waits for the last fme_refine_among* / fme_refine_topk* batch: the jobs it refused one by one. */
int fme_refine_among_status(fme_ctx* ctx);

/* d_rows: n rows; d_cand: n*k bytes. */
int fme_nn_rank_device(fme_ctx* ctx, const fme_nn_row* d_rows, uint8_t* d_cand, int k, int n, void* stream);

/* Host arrays, synchronous: cand (may be NULL) receives the n*k candidates. */
int fme_refine_topk(fme_ctx* ctx, const fme_job* jobs, fme_result* res, int k, uint8_t* cand /* may be NULL */,
                    uint32_t* cand_cost /* may be NULL */, int n, void* stream);
int fme_refine_topk_device(fme_ctx* ctx, const fme_job* d_jobs, fme_result* d_res, int k,
                           uint8_t* d_cand /* may be NULL */, uint32_t* d_cand_cost /* may be NULL */, int n,
                           void* stream);
int fme_refine_topk_mv_device(fme_ctx* ctx, const fme_job* d_jobs, fme_mv_result* d_out, int k,
                              uint8_t* d_cand /* may be NULL */, uint32_t* d_cand_cost /* may be NULL */, int n,
                              void* stream);

/* With profiling on: device milliseconds of the last among / rank / top-K call (waits for it): the
 * EMI kernel, the rows kernel, the ranking kernel, the evaluation kernel (0 for a phase the call did
 * not run), the whole call (front end included). */
int fme_among_last_ms(fme_ctx* ctx, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif /* FME_AMONG_H_ */
