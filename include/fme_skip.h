/* fme_skip.h — the skip-mode RD check of the 2Nx2N merge candidates on the GPU.
 *
 * Additional exports of libfme_amd.so beside include/fme.h and include/fme_merge.h (which this
 * header includes; they are not part of the FME_ABI_VERSION-counted set).  They cover the second
 * pass (uiNoResidual == 1) of TEncCu::xCheckRDCostMerge2Nx2N (TEncCu.cpp:1157-1282), per CU and
 * merge candidate:
 *   motionCompensation of Y, Cb and Cr (TComPrediction.cpp:495-560), exactly fme_motion_compensate
 *       without FME_MC_WP: clipMv per list against the CU origin, xCheckIdenticalMotion,
 *       xPredInterBlk (luma 8-tap quarter-pel, 4:2:0 chroma 4-tap eighth-pel), uni-prediction
 *       clipped to the bit depth, bi-prediction through 14-bit values and TComYuv::addAvg;
 *   encodeResAndCalcRdInterCU(..., bSkipResidual = true) (TEncSearch.cpp:5287-5332): per component
 *       TComRdCost::getDistPart(bitDepth, pred, org, w >> csx, h >> csy, compID) with DF_SSE
 *       (TComRdCost.cpp:327-345; xGetSSE* 861-1205: the sum over the block of
 *       (org - pred)^2 >> ((bitDepth - 8) << 1), each sample's square shifted; Distortion is UInt);
 *       Cb and Cr each weighted, (Distortion)(m_distortionWeight[compID] * sse) (:343); the CU's
 *       distortion Y + Cb' + Cr' in UInt arithmetic; calcRdCost(bits, distortion) with DF_DEFAULT
 *       in COST_STANDARD_LOSSY = (double)distortion + (double)bits * lambda (:57-102), lambda the
 *       full m_dLambda (not the motion lambda of fme_set_lambda);
 *   xCheckBestMode (TEncCu.cpp:1239): the first evaluated candidate with the strictly least cost.
 * One kernel launch computes the three SSEs of every (CU, candidate) of a batch without writing
 * prediction planes.
 *
 * What stays with the caller: the residual pass (uiNoResidual == 0) with its transform, quantiser
 * and CABAC; getInterMergeCandidates (it reads decided CUs); the bit count of each candidate
 * (transquant-bypass flag, skip flag and merge index from the caller's CABAC state,
 * TEncSearch.cpp:5305-5316); early-skip detection; lossless CUs (the reference runs no skip pass
 * for them) and the lossless cost modes; weighted prediction (a task with FME_MC_WP is invalid
 * here); chroma formats other than 4:2:0.                                                        */
#ifndef FME_SKIP_H_
#define FME_SKIP_H_

#include "fme_merge.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FME_SKIP_NONE 0xFFu      /* fme_skip_res.best: no candidate was evaluated                 */

/* One motionCompensation + getDistPart(DF_SSE) of Y, Cb and Cr: a block and one motion.  The
 * fields and their validity are fme_pe_task's, with these differences: w and h are any multiples
 * of 4 in 4..64 (every shape fme_mc_job admits); the original and each used reference must have
 * their chroma planes set (fme_set_picture_yuv) and equal dimensions; flags are FME_MC_L0 and / or
 * FME_MC_L1 only.                                                                                */
typedef struct fme_sse_task {
  uint16_t x, y;
  uint8_t  w, h;
  uint8_t  org_id;
  uint8_t  flags;
  uint16_t cu_x, cu_y;
  uint8_t  ref_id[2];
  uint16_t reserved;
  int16_t  mv[2][2];
} fme_sse_task;   /* 24 bytes */

/* sse[i] = { Y, Cb, Cr } of tasks[i], unweighted.
 * fme_pred_sse: host arrays, synchronous; a batch with any invalid task is rejected
 *   (FME_E_INVALID, nothing runs, sse is not written); n == 0 returns 0.
 * fme_pred_sse_device: device arrays, stream-ordered, no host synchronisation; an invalid task is
 *   skipped, gets 0xFFFFFFFF in all three slots and is counted; fme_pred_sse_invalid_count() waits
 *   and returns the count of the last such call.                                                 */
int fme_pred_sse(fme_ctx* ctx, const fme_sse_task* tasks, uint32_t (*sse)[3], int n, void* stream);
int fme_pred_sse_device(fme_ctx* ctx, const fme_sse_task* d_tasks, uint32_t (*d_sse)[3], int n, void* stream);
int fme_pred_sse_invalid_count(fme_ctx* ctx);
/* With profiling on: device milliseconds of the last SSE launch; waits for it. */
int fme_pred_sse_last_ms(fme_ctx* ctx, float* ms);

/* The slice-level values of one fme_skip_estimate call.  lambda: finite, >= 0; chroma_weight:
 * finite, 0..64 (the weighted SSE then fits Distortion). */
typedef struct fme_skip_params {
  double lambda;              /* m_dLambda (TComRdCost::setLambda)                                */
  double chroma_weight[2];    /* m_distortionWeight[COMPONENT_Cb], [COMPONENT_Cr] (TEncSlice.cpp:121) */
} fme_skip_params;   /* 24 bytes */

/* One CU of xCheckRDCostMerge2Nx2N's skip pass.  A request with n_cand == 0 or no masked-in
 * candidate is valid and yields "none". */
typedef struct fme_skip_req {
  uint16_t x, y;              /* CU luma rectangle; the CU is its own clipMv origin               */
  uint8_t  w, h;
  uint8_t  org_id;
  uint8_t  n_cand;            /* numValidMergeCand, 0..5                                          */
  uint8_t  cand_mask;         /* bit i set: candidate i is evaluated (clear where the residual
                                 pass found QtRootCbf == 0: mergeCandBuffer, TEncCu.cpp:1200,
                                 1231-1235); bits at and above n_cand are ignored                 */
  uint8_t  flags;             /* reserved, 0                                                      */
  uint16_t reserved;
  fme_merge_cand cand[FME_MRG_MAX_CAND];
  uint32_t bits[FME_MRG_MAX_CAND];   /* the candidate's bit count (the caller's CABAC estimate)   */
  uint32_t reserved2;
} fme_skip_req;   /* 96 bytes */

typedef struct fme_skip_res {
  double   best_cost;                      /* +inf for none                                       */
  double   cand_cost[FME_MRG_MAX_CAND];    /* +inf beyond n_cand or masked out                    */
  uint32_t cand_sse[FME_MRG_MAX_CAND][3];  /* Y, Cb, Cr unweighted; 0xFFFFFFFF beyond n_cand or masked out */
  uint32_t cand_dist[FME_MRG_MAX_CAND];    /* Y + Cb' + Cr'; 0xFFFFFFFF beyond n_cand or masked out */
  uint8_t  best;                           /* 0..4, or FME_SKIP_NONE                              */
  uint8_t  reserved[7];
} fme_skip_res;   /* 136 bytes */

/* Host arrays, synchronous: the evaluated candidates become fme_sse_tasks, one launch computes
 * them, then per request the weighting, the cost and the strict minimum on the host.  A batch with
 * any invalid request is rejected (FME_E_INVALID, nothing runs). */
int fme_skip_estimate(fme_ctx* ctx, const fme_skip_params* params, const fme_skip_req* reqs, fme_skip_res* res, int n,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FME_SKIP_H_ */
