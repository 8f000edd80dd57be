// fme_surface.cpp — the cost-surface entry points of include/fme_surface.h: host code over the
// runtime (fme_ctx.h) around one k_cost_surface launch (fme_surface.hip); the arithmetic that needs
// no GPU is in fme_surface_host.h.
#include "fme_ctx.h"
#include "fme_surface_host.h"

using namespace fme;

namespace {

// The host checks' form of k_cost_surface's sf_job_valid.
const char* surf_job_problem(const fme_ctx* c, const fme_job& j, const uint8_t* probe) {
  if (!surf_shape_ok(j.w, j.h)) return "PU size";
  if (probe && (!surf_probe_ok(probe[0]) || !surf_probe_ok(probe[1]))) return "probe index";
  if (j.ref_id >= FME_MAX_PICTURES || !c->pics[j.ref_id].luma) return "reference picture";
  if (j.lambda_id >= FME_MAX_LAMBDAS) return "lambda id";
  if (j.key_offset >= 0)
    return (size_t)j.key_offset + (size_t)j.w * j.h <= c->n_keys ? nullptr : "key block outside the key buffer";
  if (j.org_id >= FME_MAX_PICTURES || !c->pics[j.org_id].luma) return "original picture";
  const PicDesc& o = c->pics[j.org_id];
  const PicDesc& r = c->pics[j.ref_id];
  if (o.width != r.width || o.height != r.height) return "reference picture dimensions";
  if ((int)j.x + j.w > o.width || (int)j.y + j.h > o.height) return "PU outside the picture";
  return nullptr;
}

int surf_launch(fme_ctx* c, const fme_job* d_jobs, const uint8_t* d_probe, fme_surface* d_surf, fme_surface_pick* d_pick,
                int n, hipStream_t s) {
  FME_TRY(c->surf_invalid.zero(s));
  FME_TRY(sync_tables(c, s));
  SurfArgs a{};
  a.jobs = d_jobs;
  a.probe = d_probe;
  a.surf = d_surf;
  a.pick = d_pick;
  a.pics = c->d_pics.p;
  a.mlambda = c->d_mlambda.p;
  a.keys = c->d_keys.p;
  a.n_keys = (int64_t)c->n_keys;
  a.invalid = c->surf_invalid.d.p;
  a.n = n;
  a.bit_depth = c->cfg.bit_depth;
  a.use_hadamard = c->cfg.use_hadamard ? 1 : 0;
  FME_TRY(c->surf_timer.begin(c, s));
  HIP_TRY(launch_cost_surface(a, s));
  return c->surf_timer.end(c, s);
}

}  // namespace

extern "C" {

int fme_cost_surface(fme_ctx* c, const fme_job* jobs, const uint8_t (*probe)[2], fme_surface* surf, fme_surface_pick* pick,
                     int n, void* stream) {
  if (!c || n < 0 || (!surf && !pick) || (n > 0 && !jobs)) return fail(FME_E_INVALID, "fme_cost_surface: bad argument");
  for (int i = 0; i < n; i++)
    if (const char* why = surf_job_problem(c, jobs[i], probe ? probe[i] : nullptr))
      return fail(FME_E_INVALID, "fme_cost_surface: job %d: %s", i, why);
  if (n == 0) return FME_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_surf_jobs.reserve((size_t)n));
  if (probe) HIP_TRY(c->d_surf_probe.reserve(2 * (size_t)n));
  if (surf) HIP_TRY(c->d_surf_out.reserve((size_t)n));
  if (pick) HIP_TRY(c->d_surf_pick.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(c->d_surf_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  if (probe) HIP_TRY(hipMemcpyAsync(c->d_surf_probe.p, probe, 2 * (size_t)n, hipMemcpyHostToDevice, s));
  FME_TRY(surf_launch(c, c->d_surf_jobs.p, probe ? c->d_surf_probe.p : nullptr, surf ? c->d_surf_out.p : nullptr,
                      pick ? c->d_surf_pick.p : nullptr, n, s));
  if (surf) HIP_TRY(hipMemcpyAsync(surf, c->d_surf_out.p, (size_t)n * sizeof(fme_surface), hipMemcpyDeviceToHost, s));
  if (pick) HIP_TRY(hipMemcpyAsync(pick, c->d_surf_pick.p, (size_t)n * sizeof(fme_surface_pick), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

int fme_cost_surface_device(fme_ctx* c, const fme_job* d_jobs, const uint8_t (*d_probe)[2], fme_surface* d_surf,
                            fme_surface_pick* d_pick, int n, void* stream) {
  if (!c || n < 0 || (!d_surf && !d_pick) || (n > 0 && !d_jobs))
    return fail(FME_E_INVALID, "fme_cost_surface_device: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  return surf_launch(c, d_jobs, reinterpret_cast<const uint8_t*>(d_probe), d_surf, d_pick, n,
                     static_cast<hipStream_t>(stream));
}

int fme_cost_surface_invalid_count(fme_ctx* c) {
  return invalid_count(c, &fme_ctx::surf_invalid, "fme_cost_surface_invalid_count");
}

int fme_cost_surface_last_ms(fme_ctx* c, float* ms) {
  return timer_last_ms(c, &fme_ctx::surf_timer, "fme_cost_surface_last_ms", "surface launch", ms);
}

}  // extern "C"
