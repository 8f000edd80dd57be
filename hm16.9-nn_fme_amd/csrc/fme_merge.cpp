// fme_merge.cpp — the prediction-error and merge-estimation entry points of include/fme_merge.h
// (TEncSearch.cpp:3576-3655, 4110-4172): host code over the runtime (fme_ctx.h) around one
// k_pred_err launch (fme_merge.hip); the requests' arithmetic is in fme_merge_host.h.
#include "fme_ctx.h"
#include "fme_merge_host.h"

using namespace fme;

namespace {

// The host checks' form of k_pred_err's pe_task_valid.
const char* pe_task_problem(const fme_ctx* c, const fme_pe_task& t) {
  return pred_task_problem(c, kPredErr, t.x, t.y, t.w, t.h, t.flags, t.ref_id, t.org_id, 0, 0);
}

int pe_launch(fme_ctx* c, const fme_pe_task* d_tasks, uint32_t* d_dist, int n, hipStream_t s) {
  FME_TRY(c->pe_invalid.zero(s));
  FME_TRY(sync_tables(c, s));
  PeArgs a{};
  a.tasks = d_tasks;
  a.pics = c->d_pics.p;
  a.dist = d_dist;
  a.invalid = c->pe_invalid.d.p;
  a.n = n;
  a.bit_depth = c->cfg.bit_depth;
  a.use_hadamard = c->cfg.use_hadamard ? 1 : 0;
  FME_TRY(c->pe_timer.begin(c, s));
  HIP_TRY(launch_pred_err(a, s));
  return c->pe_timer.end(c, s);
}

// Validated host tasks -> their distortions: one upload, one launch, one download, one wait.
int pe_round_trip(fme_ctx* c, const fme_pe_task* tasks, uint32_t* dist, int n, hipStream_t s) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_pe_tasks.reserve((size_t)n));
  HIP_TRY(c->d_pe_dist.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(c->d_pe_tasks.p, tasks, (size_t)n * sizeof(fme_pe_task), hipMemcpyHostToDevice, s));
  FME_TRY(pe_launch(c, c->d_pe_tasks.p, c->d_pe_dist.p, n, s));
  HIP_TRY(hipMemcpyAsync(dist, c->d_pe_dist.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

}  // namespace

extern "C" {

int fme_pred_error(fme_ctx* c, const fme_pe_task* tasks, uint32_t* dist, int n, void* stream) {
  if (!c || n < 0 || (n > 0 && (!tasks || !dist))) return fail(FME_E_INVALID, "fme_pred_error: bad argument");
  for (int i = 0; i < n; i++)
    if (const char* why = pe_task_problem(c, tasks[i])) return fail(FME_E_INVALID, "fme_pred_error: task %d: %s", i, why);
  if (n == 0) return FME_OK;
  return pe_round_trip(c, tasks, dist, n, static_cast<hipStream_t>(stream));
}

int fme_pred_error_device(fme_ctx* c, const fme_pe_task* d_tasks, uint32_t* d_dist, int n, void* stream) {
  if (!c || n < 0 || (n > 0 && (!d_tasks || !d_dist))) return fail(FME_E_INVALID, "fme_pred_error_device: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  return pe_launch(c, d_tasks, d_dist, n, static_cast<hipStream_t>(stream));
}

int fme_pred_error_invalid_count(fme_ctx* c) {
  return invalid_count(c, &fme_ctx::pe_invalid, "fme_pred_error_invalid_count");
}

int fme_pred_error_last_ms(fme_ctx* c, float* ms) {
  return timer_last_ms(c, &fme_ctx::pe_timer, "fme_pred_error_last_ms", "prediction-error launch", ms);
}

int fme_merge_estimate(fme_ctx* c, const fme_merge_req* reqs, fme_merge_res* res, int n, void* stream) {
  if (!c || n < 0 || (n > 0 && (!reqs || !res))) return fail(FME_E_INVALID, "fme_merge_estimate: bad argument");
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    const fme_merge_req& q = reqs[i];
    if (const char* why = merge_req_problem(q)) return fail(FME_E_INVALID, "fme_merge_estimate: request %d: %s", i, why);
    if (q.lambda_id >= FME_MAX_LAMBDAS || !c->lambda_set[q.lambda_id])
      return fail(FME_E_INVALID, "fme_merge_estimate: request %d: lambda %d not set", i, (int)q.lambda_id);
    total += (size_t)merge_task_count(q);
  }
  if (n == 0) return FME_OK;
  if (total > (size_t)INT32_MAX) return fail(FME_E_INVALID, "fme_merge_estimate: %zu tasks", total);
  c->h_pe_tasks.resize(total);
  c->h_pe_dist.resize(total);
  size_t at = 0;
  for (int i = 0; i < n; i++) {
    const int m = merge_expand(reqs[i], c->h_pe_tasks.data() + at);
    for (int k = 0; k < m; k++)
      if (const char* why = pe_task_problem(c, c->h_pe_tasks[at + k]))
        return fail(FME_E_INVALID, "fme_merge_estimate: request %d motion %d: %s", i, k, why);
    at += (size_t)m;
  }
  FME_TRY(pe_round_trip(c, c->h_pe_tasks.data(), c->h_pe_dist.data(), (int)total, static_cast<hipStream_t>(stream)));
  at = 0;
  for (int i = 0; i < n; i++) {
    merge_decide(reqs[i], c->h_pe_dist.data() + at, c->mlambda[reqs[i].lambda_id], res[i]);
    at += (size_t)merge_task_count(reqs[i]);
  }
  return FME_OK;
}

}  // extern "C"
