// fme_extern_host.h — the arithmetic of the external-predictor path (include/fme_extern.h) that
// needs no GPU: how a row of NN inputs turns back into a record's EMI fields, which classes and
// rows refuse a job, and the argument checks of the entry points.  Plain C++ over
// include/fme_extern.h: no HIP, so a CPU test can include it alone (tests/cpp/test_extern_host.cpp);
// the kernels (fme_extern.hip) and the runtime include it too, hence FME_EXTERN_HD.
#pragma once

#include <cstdint>

#include "../../include/fme_extern.h"
#include "fme_direct_host.h"

#if defined(__HIPCC__)
#define FME_EXTERN_HD __host__ __device__ inline
#else
#define FME_EXTERN_HD inline
#endif

namespace fme {

static_assert(sizeof(fme_nn_row) == 64, "fme_nn_row layout");
static_assert((FME_RES_NN_EXTERN & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_NN_DIRECT | FME_RES_REJECTED)) == 0,
              "FME_RES_NN_EXTERN is a status bit of its own");

// A class the evaluation has a position for.
FME_EXTERN_HD bool extern_class_ok(int cls) { return cls >= 0 && cls < kDirectClasses; }

// The EMI square step moves the integer MV by at most one sample in each component, so a row whose
// MV lies farther from the job's is not this job's row.
FME_EXTERN_HD bool extern_row_mv_ok(int row_x, int row_y, int job_x, int job_y) {
  const int dx = row_x - job_x, dy = row_y - job_y;
  return dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1;
}

// A row fme_refine_at accepts for a job whose mv is (job_x, job_y).
FME_EXTERN_HD bool extern_row_ok(const fme_nn_row& r, int job_x, int job_y) {
  return !(r.status & FME_RES_REJECTED) && extern_row_mv_ok(r.mv_int_x, r.mv_int_y, job_x, job_y);
}

// The record's EMI fields from a row, every other field 0: mv_int; n_emi (at most 8); the job's own
// pushes are the row's first n_emi slots (a job pushes slots 0 .. n_emi - 1, and the row holds its
// own push wherever it pushes); C where the job wrote it.
FME_EXTERN_HD void extern_row_record(const fme_nn_row& r, fme_result& out) {
  out = fme_result{};
  const int n = r.n_emi < 8 ? r.n_emi : 8;
  out.mv_int_x = r.mv_int_x;
  out.mv_int_y = r.mv_int_y;
  out.c = r.writes ? r.c : 0u;
  for (int s = 0; s < 8; s++) out.emi[s] = s < n ? r.e[s] : 0u;
  out.n_emi = (uint8_t)n;
}

// The entry points' argument checks: 0 (run), 1 (n == 0: nothing to do) or a negative FME_E_* code.
// bound: NN input rows are bound to the context (fme_set_nn_inputs).
inline int extern_inputs_request(const void* ctx, const void* jobs, const void* rows, int n, bool bound) {
  if (!ctx || n < 0 || (n > 0 && (!jobs || !rows))) return FME_E_INVALID;
  if (bound) return FME_E_STATE;
  return n == 0 ? 1 : 0;
}
inline int extern_at_request(const void* ctx, const void* jobs, const void* cls, const void* out, int n, bool bound) {
  if (!ctx || n < 0 || (n > 0 && (!jobs || !cls || !out))) return FME_E_INVALID;
  if (bound) return FME_E_STATE;
  return n == 0 ? 1 : 0;
}

// The host-array form's check before anything is enqueued: the first job a batch would refuse, or -1.
inline int extern_first_refused(const fme_job* jobs, const fme_nn_row* rows, const uint8_t* cls, int n) {
  for (int i = 0; i < n; i++) {
    if (!extern_class_ok(cls[i])) return i;
    if (rows && !extern_row_ok(rows[i], jobs[i].mv_x, jobs[i].mv_y)) return i;
  }
  return -1;
}

}  // namespace fme
