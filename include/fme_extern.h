/* fme_extern.h — an external sub-pel predictor: the NN inputs of every job out as device rows, one
 * class per job in from a device array.
 *
 * Additional exports of libfme_amd.so beside include/fme.h (they are not part of the
 * FME_ABI_VERSION-counted set).  An NN-direct batch (include/fme_direct.h) is the EMI step, the
 * net, and one sub-pel evaluation at the net's class.  The two families here are that batch split
 * at the class: fme_nn_inputs* runs the EMI step and hands out what NN_pred() would read for every
 * job, resolved (stale slots, carried C / PU size) and advances the carried NN state;
 * fme_refine_at* takes one class per job from the caller and finishes the records.  Whatever sits
 * between them on the same stream is the predictor: a torch module, a table, the true minimum of
 * fme_cost_surface_device.  Neither family needs a loaded net: both work in every nn_mode.
 *
 * fme_nn_inputs*: row i holds exactly what the NN tail resolves for job i before it calls the net:
 *   e[s]        the job's own push where it pushes slot s, else that of the last earlier job of the
 *               batch that pushes s, else the incoming state's; under a loaded net with
 *               FME_NN_IN_SLOT_RESET: the job's own push, else 0;
 *   c, pu_h, pu_w   of the last job at or before i with FME_JOB_EMI, else the incoming state's;
 *   mv_int_*, n_emi  the job's own EMI step (fme_result's fields of the same names);
 *   writes      1: the job has FME_JOB_EMI;
 *   status      FME_RES_NN_STALE / FME_RES_NN_UNINIT by the tail's two conditions (in every nn_mode).
 *   The carried NN state (12 words) is left as the reference model leaves it after refining the same
 *   jobs: what fme_refine leaves in nn_mode 1 and 2; in nn_mode 0, where fme_refine carries no
 *   state, the same last-writer rule applied all the same.  So input batches, ordinary batches and
 *   direct batches interleave, and fme_nn_inputs followed by fme_refine_at over the same jobs leaves
 *   the state one fme_refine_direct leaves.  A pending fme_nn_set_state / fme_nn_reset_state is
 *   applied first.
 *   A rejected batch (an invalid job): every row is 0 but for status = FME_RES_REJECTED, the state
 *   is carried through unchanged, fme_refine_status() returns the count.
 *
 * fme_refine_at*: the record of job i,
 *   mv_int_*, c, emi[], n_emi   fme_refine's (rows == NULL: the EMI step runs); with rows they come
 *               from the row: mv_int; n_emi; emi[s] = e[s] for s < n_emi, else 0; c where writes,
 *               else 0.  With fme_nn_inputs' own rows both forms give identical records;
 *   nn_class    cls[i];
 *   half_*, qtr_*, mv_*, frac_cost, bits, cost   fme_refine_direct's for that class: frac_cost is
 *               fme_surface.cost[cls[i]] of the surface centred on mv_int;
 *   status      FME_RES_NN_DIRECT | FME_RES_NN_EXTERN.
 *   The NN state is neither read nor written, and a pending set / reset stays pending.
 *   Jobs refused one by one: a class above 48, or a row that is marked FME_RES_REJECTED or whose
 *   integer MV is more than one sample from the job's mv in either component (no EMI step moves it
 *   farther).  Such a job's record is 0 but for status = FME_RES_REJECTED, the other jobs are
 *   unaffected, and fme_refine_at_status() counts them.  An invalid job rejects the whole batch as
 *   in fme_refine_device (fme_refine_status()).
 *
 * While NN input rows are bound (fme_set_nn_inputs non-NULL) both families return FME_E_STATE: the
 * inputs are the caller's already.  With none bound an FME_JOB_NN_IN job is invalid.
 *
 * Ordering: both are planned like a direct batch: behind every refinement batch in flight, and
 * every later batch behind them.                                                                */
#ifndef FME_EXTERN_H_
#define FME_EXTERN_H_

#include "fme.h"
#include "fme_direct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_RES_NN_EXTERN 0x08u   /* nn_class was the caller's */

typedef struct fme_nn_row {        /* 64 bytes */
  uint32_t e[8];                   /* array_e[0..7] as NN_pred() reads them for this job */
  uint32_t c, pu_h, pu_w;          /* C, PUHeight, PUWidth, likewise */
  int16_t  mv_int_x, mv_int_y;     /* integer MV after the EMI step */
  uint8_t  n_emi;                  /* this job's own pushes, 0..8 */
  uint8_t  writes;                 /* 1: the job has FME_JOB_EMI (it wrote C / the PU size) */
  uint16_t status;                 /* FME_RES_NN_STALE / _UNINIT as fme_refine sets them; FME_RES_REJECTED */
  uint32_t reserved[3];            /* 0 */
} fme_nn_row;

/* Host arrays, synchronous: a batch that holds an invalid job returns FME_E_INVALID (the rows are
 * then those of a rejected batch, the NN state unchanged); n == 0 returns 0. */
int fme_nn_inputs(fme_ctx* ctx, const fme_job* jobs, fme_nn_row* rows, int n, void* stream);
/* Device arrays, stream-ordered, no host synchronisation. */
int fme_nn_inputs_device(fme_ctx* ctx, const fme_job* d_jobs, fme_nn_row* d_rows, int n, void* stream);

/* Host arrays, synchronous.  The classes (and, with rows, the rows' MVs) are checked before anything
 * is enqueued: FME_E_INVALID, res untouched. */
int fme_refine_at(fme_ctx* ctx, const fme_job* jobs, const fme_nn_row* rows /* may be NULL */,
                  const uint8_t* cls, fme_result* res, int n, void* stream);
/* Device arrays, stream-ordered, no host synchronisation. */
int fme_refine_at_device(fme_ctx* ctx, const fme_job* d_jobs, const fme_nn_row* d_rows /* may be NULL */,
                         const uint8_t* d_cls, fme_result* d_res, int n, void* stream);
/* The same with the 16-byte records of fme_refine_mv_device. */
int fme_refine_at_mv_device(fme_ctx* ctx, const fme_job* d_jobs, const fme_nn_row* d_rows /* may be NULL */,
                            const uint8_t* d_cls, fme_mv_result* d_out, int n, void* stream);
/* Waits for the last fme_refine_at* batch: the jobs it refused one by one (0 before the first). */
int fme_refine_at_status(fme_ctx* ctx);
/* With profiling on: device milliseconds of the last call of either family (waits for it): the EMI
 * kernel, the rows kernel, the evaluation kernel (0 for a phase the call did not run), the whole
 * batch (front end included). */
int fme_extern_last_ms(fme_ctx* ctx, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* FME_EXTERN_H_ */
