/* fme_merge.h — prediction error and merge estimation of predInterSearch's PU loop on the GPU.
 *
 * Additional exports of libfme_amd.so beside include/fme.h (which this header includes; they are
 * not part of the FME_ABI_VERSION-counted set).  They replace the part of the PU loop between the
 * uni / bi decision (fme_pred_inter_p / fme_pred_inter_b) and the final motionCompensation
 * (fme_motion_compensate), TEncSearch.cpp:4110-4172:
 *   xGetInterPredictionError (3576-3596): luma motionCompensation of the PU's motion (clipMv,
 *       xPredInterBlk uni / bi, addAvg, xCheckIdenticalMotion) and the distortion against the
 *       original through setDistParam(..., bHadamard) (TComRdCost.cpp:277-290): xGetHADs
 *       (1428-1494; 8x8 Hadamards when width and height are multiples of 8, else 4x4) with HADME
 *       on and the CU not lossless, else the full SAD; the PU's sum shifted right by
 *       bitDepth - 8 (DISTORTION_PRECISION_ADJUSTMENT);
 *   xMergeEstimation (3599-3655) over the caller's merge candidates, after
 *       xRestrictBipredMergeCand (3665-3679);
 *   the uiMRGCost < uiMECost choice (4126-4171).
 * One kernel launch computes every (PU, motion) distortion of a batch without writing prediction
 * planes.  What stays with the caller: getInterMergeCandidates (it reads decided CUs), the
 * residual pass of TEncCu's 2Nx2N merge RD check (its skip pass is include/fme_skip.h), and
 * weighted prediction (bApplyWeight is false here; the prediction is the unweighted one).       */
#ifndef FME_MERGE_H_
#define FME_MERGE_H_

#include "fme.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_PE_LOSSLESS  0x04u   /* CU transquant bypass: plain SAD even with HADME on           */
#define FME_MRG_HAS_ME   0x08u   /* fme_merge_req: the ME result is set (bTestNormalMC)          */
#define FME_MRG_MAX_CAND 5       /* MRG_MAX_NUM_CANDS                                            */

/* One xGetInterPredictionError: a PU and one motion.  Validity as for fme_mc_job, but only the
 * luma planes are needed; the original and the references must have equal dimensions.
 *   flags      FME_MC_L0 and/or FME_MC_L1 (both: bi-prediction), FME_PE_LOSSLESS
 *   ref_id[l]  picture slot of list l's reference;  mv[l] quarter-pel (hor, ver)
 *   cu_x, cu_y luma origin of the CU (clipMv bounds)                                             */
typedef struct fme_pe_task {
  uint16_t x, y;
  uint8_t  w, h;
  uint8_t  org_id;
  uint8_t  flags;
  uint16_t cu_x, cu_y;
  uint8_t  ref_id[2];
  uint16_t reserved;
  int16_t  mv[2][2];
} fme_pe_task;   /* 24 bytes */

/* dist[i] = the distortion of tasks[i].
 * fme_pred_error: host arrays, synchronous; a batch with any invalid task is rejected
 *   (FME_E_INVALID, nothing runs); n == 0 returns 0.
 * fme_pred_error_device: device arrays, stream-ordered, no host synchronisation; an invalid task
 *   is skipped, gets 0xFFFFFFFF and is counted; fme_pred_error_invalid_count() waits and returns
 *   the count of the last such call.                                                             */
int fme_pred_error(fme_ctx* ctx, const fme_pe_task* tasks, uint32_t* dist, int n, void* stream);
int fme_pred_error_device(fme_ctx* ctx, const fme_pe_task* d_tasks, uint32_t* d_dist, int n, void* stream);
int fme_pred_error_invalid_count(fme_ctx* ctx);
/* With profiling on: device milliseconds of the last prediction-error launch; waits for it. */
int fme_pred_error_last_ms(fme_ctx* ctx, float* ms);

typedef struct fme_merge_cand {
  uint8_t  inter_dir;         /* uhInterDirNeighbours: 1 L0, 2 L1, 3 bi                           */
  uint8_t  ref_id[2];         /* picture slot of each used list's reference                       */
  uint8_t  reserved;
  int16_t  mv[2][2];          /* cMvFieldNeighbours, quarter-pel (hor, ver)                       */
} fme_merge_cand;   /* 12 bytes */

/* One non-2Nx2N PU of TEncSearch.cpp:4110-4172.  A request with neither a candidate nor an ME
 * result is invalid. */
typedef struct fme_merge_req {
  uint16_t x, y;              /* PU luma rectangle                                                */
  uint8_t  w, h;
  uint8_t  org_id;
  uint8_t  lambda_id;         /* motion lambda (fme_set_lambda / fme_set_motion_lambda)           */
  uint16_t cu_x, cu_y;        /* CU luma origin                                                   */
  uint8_t  cu_w;              /* CU width (isBipredRestriction: 8 and a PU side < 8)              */
  uint8_t  max_num_merge_cand;/* getMaxNumMergeCand, 1..5                                         */
  uint8_t  n_cand;            /* numValidMergeCand, 0..5                                          */
  uint8_t  flags;             /* FME_PE_LOSSLESS, FME_MRG_HAS_ME                                  */
  fme_merge_cand cand[FME_MRG_MAX_CAND];
  uint8_t  me_inter_dir;      /* the ME result (FME_MRG_HAS_ME): 1 / 2 / 3                        */
  uint8_t  me_ref_id[2];
  uint8_t  reserved;
  int16_t  me_mv[2][2];
  uint32_t me_bits;           /* uiMEBits                                                         */
  uint32_t reserved2;
} fme_merge_req;   /* 96 bytes */

typedef struct fme_merge_res {
  uint8_t  use_merge;         /* uiMRGCost < uiMECost (strict; uiMECost is UINT_MAX without ME)   */
  uint8_t  merge_idx;         /* uiMRGIndex (0 without candidates)                                */
  uint8_t  merge_inter_dir;   /* uiMRGInterDir after the bi-pred restriction (0 without)          */
  uint8_t  inter_dir;         /* the decided motion: merge's when use_merge, else the ME result   */
  uint8_t  ref_id[2];         /* unused list: 0                                                   */
  uint16_t reserved;
  int16_t  mv[2][2];          /* unused list: 0                                                   */
  uint32_t merge_cost;        /* uiMRGCost (0xFFFFFFFF without candidates)                        */
  uint32_t cand_dist[FME_MRG_MAX_CAND];   /* 0xFFFFFFFF beyond n_cand                             */
  uint32_t cand_cost[FME_MRG_MAX_CAND];
  uint32_t me_dist, me_cost;  /* uiMEError, uiMECost (0xFFFFFFFF without FME_MRG_HAS_ME)           */
  uint32_t cost;              /* the decided motion's cost                                        */
} fme_merge_res;   /* 72 bytes */

/* Host arrays, synchronous: the requests' motions become fme_pe_tasks, one launch computes them,
 * then per request: uiBitsCand = idx + 1 (minus 1 at idx == max_num_merge_cand - 1), cost = dist +
 * (uint32_t)(motion_lambda * bits / 65536.0) (getCost), the first candidate with the strictly least
 * cost, and use_merge = uiMRGCost < uiMECost.  A batch with any invalid request is rejected. */
int fme_merge_estimate(fme_ctx* ctx, const fme_merge_req* reqs, fme_merge_res* res, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FME_MERGE_H_ */
