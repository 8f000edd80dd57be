// fme_skip.cpp — the SSE and skip-check entry points of include/fme_skip.h (the uiNoResidual == 1
// pass of TEncCu::xCheckRDCostMerge2Nx2N, TEncCu.cpp:1157-1282): host code over the runtime
// (fme_ctx.h) around one k_pred_sse launch (fme_skip.hip); the requests' arithmetic is in
// fme_skip_host.h.
#include "fme_ctx.h"
#include "fme_skip_host.h"

using namespace fme;

namespace {

// The host checks' form of k_pred_sse's sse_task_valid.
const char* sse_task_problem(const fme_ctx* c, const fme_sse_task& t) {
  return pred_task_problem(c, kPredSse, t.x, t.y, t.w, t.h, t.flags, t.ref_id, t.org_id, 0, 0);
}

int sse_launch(fme_ctx* c, const fme_sse_task* d_tasks, uint32_t* d_sse, int n, hipStream_t s) {
  FME_TRY(c->sse_invalid.zero(s));
  FME_TRY(sync_tables(c, s));
  SseArgs a{};
  a.tasks = d_tasks;
  a.pics = c->d_pics.p;
  a.sse = d_sse;
  a.invalid = c->sse_invalid.d.p;
  a.n = n;
  a.bit_depth = c->cfg.bit_depth;
  FME_TRY(c->sse_timer.begin(c, s));
  HIP_TRY(launch_pred_sse(a, s));
  return c->sse_timer.end(c, s);
}

// Validated host tasks -> their SSEs: one upload, one launch, one download, one wait.
int sse_round_trip(fme_ctx* c, const fme_sse_task* tasks, uint32_t* sse, int n, hipStream_t s) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_sse_tasks.reserve((size_t)n));
  HIP_TRY(c->d_sse_out.reserve(3 * (size_t)n));
  HIP_TRY(hipMemcpyAsync(c->d_sse_tasks.p, tasks, (size_t)n * sizeof(fme_sse_task), hipMemcpyHostToDevice, s));
  FME_TRY(sse_launch(c, c->d_sse_tasks.p, c->d_sse_out.p, n, s));
  HIP_TRY(hipMemcpyAsync(sse, c->d_sse_out.p, 3 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

}  // namespace

extern "C" {

int fme_pred_sse(fme_ctx* c, const fme_sse_task* tasks, uint32_t (*sse)[3], int n, void* stream) {
  if (!c || n < 0 || (n > 0 && (!tasks || !sse))) return fail(FME_E_INVALID, "fme_pred_sse: bad argument");
  for (int i = 0; i < n; i++)
    if (const char* why = sse_task_problem(c, tasks[i])) return fail(FME_E_INVALID, "fme_pred_sse: task %d: %s", i, why);
  if (n == 0) return FME_OK;
  return sse_round_trip(c, tasks, &sse[0][0], n, static_cast<hipStream_t>(stream));
}

int fme_pred_sse_device(fme_ctx* c, const fme_sse_task* d_tasks, uint32_t (*d_sse)[3], int n, void* stream) {
  if (!c || n < 0 || (n > 0 && (!d_tasks || !d_sse))) return fail(FME_E_INVALID, "fme_pred_sse_device: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  return sse_launch(c, d_tasks, reinterpret_cast<uint32_t*>(d_sse), n, static_cast<hipStream_t>(stream));
}

int fme_pred_sse_invalid_count(fme_ctx* c) {
  return invalid_count(c, &fme_ctx::sse_invalid, "fme_pred_sse_invalid_count");
}

int fme_pred_sse_last_ms(fme_ctx* c, float* ms) {
  return timer_last_ms(c, &fme_ctx::sse_timer, "fme_pred_sse_last_ms", "SSE launch", ms);
}

int fme_skip_estimate(fme_ctx* c, const fme_skip_params* params, const fme_skip_req* reqs, fme_skip_res* res, int n,
                      void* stream) {
  if (!c || !params || n < 0 || (n > 0 && (!reqs || !res))) return fail(FME_E_INVALID, "fme_skip_estimate: bad argument");
  if (const char* why = skip_params_problem(*params)) return fail(FME_E_INVALID, "fme_skip_estimate: params: %s", why);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    if (const char* why = skip_req_problem(reqs[i])) return fail(FME_E_INVALID, "fme_skip_estimate: request %d: %s", i, why);
    total += (size_t)skip_task_count(reqs[i]);
  }
  if (n == 0) return FME_OK;
  if (total > (size_t)INT32_MAX) return fail(FME_E_INVALID, "fme_skip_estimate: %zu tasks", total);
  c->h_sse_tasks.resize(total);
  c->h_sse_out.resize(3 * total);
  size_t at = 0;
  for (int i = 0; i < n; i++) {
    const int m = skip_expand(reqs[i], c->h_sse_tasks.data() + at);
    for (int k = 0; k < m; k++)
      if (const char* why = sse_task_problem(c, c->h_sse_tasks[at + k]))
        return fail(FME_E_INVALID, "fme_skip_estimate: request %d motion %d: %s", i, k, why);
    at += (size_t)m;
  }
  if (total > 0)   // a batch whose requests evaluate no candidate launches nothing
    FME_TRY(sse_round_trip(c, c->h_sse_tasks.data(), c->h_sse_out.data(), (int)total, static_cast<hipStream_t>(stream)));
  at = 0;
  for (int i = 0; i < n; i++) {
    skip_decide(reqs[i], *params, reinterpret_cast<const uint32_t(*)[3]>(c->h_sse_out.data() + 3 * at), res[i]);
    at += (size_t)skip_task_count(reqs[i]);
  }
  return FME_OK;
}

}  // extern "C"
