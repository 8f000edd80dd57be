// fme_producers.cpp — predInterSearch's PU / reference loops: the P-slice and
// B-slice producers fme_pred_inter_p / fme_pred_inter_b, and the stages they share with the public
// ABI (fme_template_costs, fme_build_bipred_keys*).  Host code over the runtime (fme_ctx.h); the
// arithmetic and the steps both producers share are in fme_pi_host.h.
#include <chrono>

#include "fme_ctx.h"
#include "fme_pi_host.h"

using namespace fme;

namespace {

// A known PU shape inside the bound picture slot org_id.
bool valid_pu(const fme_ctx* c, int org_id, int x, int y, int w, int h) {
  int k = 0;
  while (k < kNumClasses && (kClassW[k] != w || kClassH[k] != h)) k++;   // stops at the shape's class
  return k < kNumClasses && org_id < FME_MAX_PICTURES && c->pics[org_id].luma && x + w <= c->pics[org_id].width &&
         y + h <= c->pics[org_id].height;
}
// Reference slot rid of a PU on slot org_id: bound, and of the original's size.
bool valid_ref(const fme_ctx* c, int org_id, int rid) {
  return rid < FME_MAX_PICTURES && c->pics[rid].luma && c->pics[rid].width == c->pics[org_id].width &&
         c->pics[rid].height == c->pics[org_id].height;
}

// The template SADs (xGetTemplateCost) of the ntasks AmvpTasks in c->h_pi_tasks, into c->h_pi_tsad:
// one upload, one launch, one download, one synchronisation.
int amvp_round_trip(fme_ctx* c, int ntasks, hipStream_t s) {
  if (ntasks <= 0) return FME_OK;
  HIP_TRY(c->d_amvp.reserve((size_t)ntasks));
  HIP_TRY(c->d_amvp_sad.reserve((size_t)ntasks));
  HIP_TRY(hipMemcpyAsync(c->d_amvp.p, c->h_pi_tasks.p, (size_t)ntasks * sizeof(AmvpTask), hipMemcpyHostToDevice, s));
  AmvpArgs aa{c->d_amvp.p, c->d_pics.p, c->d_amvp_sad.p, (int32_t)ntasks, c->cfg.bit_depth};
  HIP_TRY(launch_amvp_sad(aa, s));
  HIP_TRY(hipMemcpyAsync(c->h_pi_tsad.p, c->d_amvp_sad.p, (size_t)ntasks * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

void mv_copy(int16_t dst[2], const int16_t src[2]) { dst[0] = src[0]; dst[1] = src[1]; }

// The uni-pred search job of request q on reference slot ref_id: xSetSearchRange around its AMVP predictor.
template <typename Req>
void uni_job(const fme_ctx* c, const Req& q, uint8_t ref_id, const int16_t pred[2], uint32_t bits_in, fme_job& j,
             fme_tz_ext& e) {
  search_job(q, c->pics[q.org_id].width, c->pics[q.org_id].height, ref_id, pred, pred[0], pred[1],
             q.search_range ? q.search_range : 64, FME_JOB_EMI, bits_in, -1, reads_2n(q), j, e);
}

template <typename Req>
AmvpTask amvp_task(const Req& q, uint8_t ref_id, const int16_t cand[2]) {
  return AmvpTask{q.x, q.y, q.w, q.h, q.org_id, ref_id, q.cu_x, q.cu_y, cand[0], cand[1]};
}

// The producers' integer searches by m_integerMv2Nx2N dependency level.  jobs / ext: pinned host
// arrays in request order; src[u]: the job whose post-EMI MV job u reads (-1: none); lvl[u] its
// level (assign_levels).  The jobs go to the device once, are reordered there by level (level_order)
// for k_tz_level's launches, and come back in request order in c->d_jobs for the sub-pel pass;
// nothing returns to the host.
int tz_levels_device(fme_ctx* c, const fme_job* jobs, const fme_tz_ext* ext, const int* src, const int* lvl, int nj,
                     int max_level, hipStream_t s) {
  if (nj <= 0) return FME_OK;
  HIP_TRY(c->h_pi_idx.reserve((size_t)2 * nj));
  HIP_TRY(c->h_pi_psrc.reserve((size_t)nj));
  int32_t* const order = c->h_pi_idx.p;        // level position -> job
  int32_t* const pos = c->h_pi_idx.p + nj;     // job -> level position
  int32_t* const psrc = c->h_pi_psrc.p;
  level_order(jobs, lvl, nj, max_level, c->pi_off, c->pi_fill, c->pi_start, c->pi_byarea, order, pos);
  par_for(nj, [&](int lo, int hi) { level_psrc(src, order, pos, lo, hi, psrc); });
  HIP_TRY(c->d_jobs.reserve(nj));
  HIP_TRY(c->d_tz_ext.reserve(nj));
  HIP_TRY(c->d_pi_jobs.reserve(nj));
  HIP_TRY(c->d_pi_ext.reserve(nj));
  HIP_TRY(c->d_pi_idx.reserve((size_t)2 * nj));
  HIP_TRY(c->d_ch_i32.reserve(nj));
  HIP_TRY(c->d_tz_emi.reserve((size_t)2 * nj));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)nj * sizeof(fme_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_tz_ext.p, ext, (size_t)nj * sizeof(fme_tz_ext), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_pi_idx.p, order, (size_t)2 * nj * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_ch_i32.p, psrc, (size_t)nj * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_gather_jobs(c->d_jobs.p, c->d_tz_ext.p, c->d_pi_idx.p, c->d_pi_jobs.p, c->d_pi_ext.p, nj, s));
  TzArgs ta{};
  ta.a = batch_args(c, c->d_pi_jobs.p, nj);
  ta.jobs_out = c->d_pi_jobs.p;
  ta.ext = c->d_pi_ext.p;
  ta.ext_stride = (int)sizeof(fme_tz_ext);
  ta.emi_mv = c->d_tz_emi.p;
  const TzChain ch{c->d_ch_i32.p, max_level + 1};
  HIP_TRY(launch_tz_levels(ta, ch, c->pi_off.data(), c->cfg.bit_depth, s));
  // the searched jobs back in request order for the sub-pel pass, on the device
  HIP_TRY(launch_gather_jobs(c->d_pi_jobs.p, nullptr, c->d_pi_idx.p + nj, c->d_jobs.p, nullptr, nj, s));
  return FME_OK;
}

// Phase clock of the producers (fme_pred_inter_phases): lap(k) adds the time since the last lap to
// phase k.
struct PiClock {
  fme_ctx* c;
  std::chrono::steady_clock::time_point t0, t;
  explicit PiClock(fme_ctx* cc) : c(cc), t0(std::chrono::steady_clock::now()), t(t0) {
    for (double& v : c->pi_ms) v = 0.0;
  }
  void lap(int k) {
    const auto now = std::chrono::steady_clock::now();
    c->pi_ms[k] += std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
  }
  ~PiClock() { c->pi_ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace

extern "C" {

// xGetTemplateCost (TEncSearch.cpp:4397-4436) of every AMVP candidate of every request, one launch:
// costs[(i * FME_MAX_REFS + k) * 2 + m]; 0xFFFFFFFF for k >= num_refs or m >= n_cand[k].
int fme_template_costs(fme_ctx* c, const fme_pu_req* reqs, uint32_t* costs, int n, void* stream) {
  if (!c || (n > 0 && (!reqs || !costs))) return fail(FME_E_INVALID, "fme_template_costs: null argument");
  if (n <= 0) return n == 0 ? FME_OK : fail(FME_E_INVALID, "fme_template_costs: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<int> slot;
  for (int i = 0; i < n; i++) {
    const fme_pu_req& q = reqs[i];
    if (!valid_pu(c, q.org_id, q.x, q.y, q.w, q.h) || q.num_refs < 1 || q.num_refs > FME_MAX_REFS ||
        q.lambda_id >= FME_MAX_LAMBDAS || !c->lambda_set[q.lambda_id])
      return fail(FME_E_INVALID, "fme_template_costs: request %d invalid", i);
    for (int k = 0; k < FME_MAX_REFS; k++)
      for (int m = 0; m < 2; m++) {
        costs[((size_t)i * FME_MAX_REFS + k) * 2 + m] = 0xFFFFFFFFu;
        if (k >= q.num_refs || m >= q.n_cand[k]) continue;
        if (q.n_cand[k] > 2 || !valid_ref(c, q.org_id, q.ref_id[k]))
          return fail(FME_E_INVALID, "fme_template_costs: request %d reference %d invalid", i, k);
        slot.push_back((i * FME_MAX_REFS + k) * 2 + m);
      }
  }
  if (slot.empty()) return FME_OK;
  FME_TRY(sync_tables(c, s));
  const int ntasks = (int)slot.size();
  HIP_TRY(c->h_pi_tasks.reserve((size_t)ntasks));
  HIP_TRY(c->h_pi_tsad.reserve((size_t)ntasks));
  for (int t = 0; t < ntasks; t++) {
    const fme_pu_req& q = reqs[slot[t] / (2 * FME_MAX_REFS)];
    const int k = (slot[t] >> 1) % FME_MAX_REFS;
    c->h_pi_tasks.p[t] = amvp_task(q, q.ref_id[k], q.cand[k][slot[t] & 1]);
  }
  FME_TRY(amvp_round_trip(c, ntasks, s));
  for (int t = 0; t < ntasks; t++)
    costs[slot[t]] = template_cost(c->h_pi_tsad.p[t], slot[t] & 1, c->mlambda[reqs[slot[t] / (2 * FME_MAX_REFS)].lambda_id]);
  return FME_OK;
}

int fme_build_bipred_keys(fme_ctx* c, const fme_bikey_req* reqs, int n, size_t key_count, void* stream) {
  static_assert(sizeof(fme_bikey_req) == sizeof(BiKeyTask), "fme_bikey_req is the kernel's task record");
  if (!c || (n > 0 && !reqs)) return fail(FME_E_INVALID, "fme_build_bipred_keys: null argument");
  if (n < 0) return fail(FME_E_INVALID, "fme_build_bipred_keys: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n; i++) {
    const fme_bikey_req& q = reqs[i];
    if (!valid_pu(c, q.org_id, q.x, q.y, q.w, q.h) || !valid_ref(c, q.org_id, q.ref_id) || q.key_offset < 0 ||
        (q.key_offset & 3) || (size_t)q.key_offset + (size_t)q.w * q.h > key_count || (q.flags & ~FME_PU_CLIP_BIPRED))
      return fail(FME_E_INVALID, "fme_build_bipred_keys: request %d invalid", i);
  }
  FME_TRY(sync_tables(c, s));
  FME_TRY(grow_keys(c, key_count));
  c->n_keys = key_count;
  HIP_TRY(hipMemsetAsync(c->d_key_invalid.p, 0, sizeof(int32_t), s));   // host-validated: the keys are good
  if (n == 0) return hipStreamSynchronize(s) == hipSuccess ? FME_OK : fail(FME_E_DEVICE, "fme_build_bipred_keys: sync");
  HIP_TRY(c->d_bikey.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(c->d_bikey.p, reqs, (size_t)n * sizeof(BiKeyTask), hipMemcpyHostToDevice, s));
  BiKeyArgs ka{c->d_bikey.p, c->d_pics.p, c->d_keys.p, (int32_t)n, nullptr, (int64_t)key_count, c->cfg.bit_depth};
  HIP_TRY(launch_bi_key(ka, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

// The frame replay's per-frame form: requests already in device memory, everything stream-ordered
// (no host synchronisation).  Validation runs in k_bi_key; a request that fails it is skipped and
// counted, and every later batch whose jobs read keys is rejected until keys are built again.
int fme_build_bipred_keys_device(fme_ctx* c, const fme_bikey_req* d_reqs, int n, size_t key_count, void* stream) {
  if (!c || (n > 0 && !d_reqs)) return fail(FME_E_INVALID, "fme_build_bipred_keys_device: null argument");
  if (n < 0) return fail(FME_E_INVALID, "fme_build_bipred_keys_device: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FME_TRY(sync_tables(c, s));
  FME_TRY(grow_keys(c, key_count));   // growing frees the old buffer: this context's queued batches finish first
  c->n_keys = key_count;
  HIP_TRY(hipMemsetAsync(c->d_key_invalid.p, 0, sizeof(int32_t), s));
  if (n == 0) return FME_OK;
  BiKeyArgs ka{reinterpret_cast<const BiKeyTask*>(d_reqs), c->d_pics.p, c->d_keys.p, (int32_t)n,
               c->d_key_invalid.p, (int64_t)key_count, c->cfg.bit_depth};
  HIP_TRY(launch_bi_key(ka, s));
  return FME_OK;
}

int fme_pred_inter_phases(fme_ctx* c, double* ms, int count) {
  if (!c || (count > 0 && !ms)) return fail(FME_E_INVALID, "fme_pred_inter_phases: null argument");
  for (int i = 0; i < count && i < FME_PI_PHASES; i++) ms[i] = c->pi_ms[i];
  return FME_OK;
}

int fme_pred_inter_reset(fme_ctx* c) {
  if (!c) return fail(FME_E_INVALID, "fme_pred_inter_reset: null ctx");
  std::memset(c->int_mv_2n, 0, sizeof(c->int_mv_2n));
  return FME_OK;
}

// The requests run in call order as far as anything observable goes; the GPU sees them as
//   1. one AMVP template-cost launch over every (request, reference, candidate) with two candidates;
//   2. integer searches by dependency level: a request that reads m_integerMv2Nx2N[k] waits for the
//      level of the 2Nx2N request that last wrote it (per CTU the chain of 2Nx2N CUs in xCompressCU
//      order); the search kernels also run the EMI square step and return the post-EMI integer MV
//      that the 2Nx2N requests publish to the levels above;
//   3. one fme_refine over all jobs in request order (the NN's carried state as in the reference);
//   4. xCheckBestMVP and the reference choice on the host.
int fme_pred_inter_p(fme_ctx* c, const fme_pu_req* reqs, fme_pu_res* res, int n, void* stream) {
  if (!c || (n > 0 && (!reqs || !res))) return fail(FME_E_INVALID, "fme_pred_inter_p: null argument");
  if (n <= 0) return n == 0 ? FME_OK : fail(FME_E_INVALID, "fme_pred_inter_p: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  PiClock clk(c);
  // ---- validation (nothing runs on a bad batch) ----
  for (int i = 0; i < n; i++) {
    const fme_pu_req& q = reqs[i];
    if (!valid_pu(c, q.org_id, q.x, q.y, q.w, q.h) || q.part_size > FME_PART_nRx2N || q.num_refs < 1 ||
        q.num_refs > FME_MAX_REFS || q.lambda_id >= FME_MAX_LAMBDAS || !c->lambda_set[q.lambda_id] ||
        (q.flags & ~FME_PU_LOSSLESS))
      return fail(FME_E_INVALID, "fme_pred_inter_p: request %d invalid (shape %dx%d, part %d, refs %d)", i, q.w, q.h,
                  q.part_size, q.num_refs);
    for (int k = 0; k < q.num_refs; k++) {
      if (q.ref_id[k] >= FME_MAX_PICTURES || !c->pics[q.ref_id[k]].luma || q.n_cand[k] < 1 || q.n_cand[k] > 2)
        return fail(FME_E_INVALID, "fme_pred_inter_p: request %d reference %d invalid", i, k);
      if (!valid_ref(c, q.org_id, q.ref_id[k]))
        return fail(FME_E_INVALID, "fme_pred_inter_p: request %d reference %d size differs from the original", i, k);
    }
  }
  FME_TRY(sync_tables(c, s));
  // ---- 1. xEstimateMvPredAMVP template costs: two tasks per (request, reference) with two
  // candidates, built into pinned memory by the host threads ----
  std::vector<int>& base = c->pi_base;
  std::vector<int>& task_of = c->pi_task;
  base.resize((size_t)n + 1);
  base[0] = 0;
  for (int i = 0; i < n; i++) base[i + 1] = base[i] + reqs[i].num_refs;
  const int nj = base[n];
  task_of.resize((size_t)nj);
  int ntasks = 0;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < reqs[i].num_refs; k++) {
      const bool two = reqs[i].n_cand[k] >= 2;
      task_of[base[i] + k] = two ? ntasks : -1;
      ntasks += two ? 2 : 0;
    }
  HIP_TRY(c->h_pi_tasks.reserve((size_t)ntasks));
  HIP_TRY(c->h_pi_tsad.reserve((size_t)ntasks));
  AmvpTask* const tasks = c->h_pi_tasks.p;
  const uint32_t* const tsad = c->h_pi_tsad.p;
  par_for(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; i++) {
      const fme_pu_req& q = reqs[i];
      for (int k = 0; k < q.num_refs; k++) {
        const int t = task_of[base[i] + k];
        if (t < 0) continue;
        for (int m = 0; m < 2; m++) tasks[t + m] = amvp_task(q, q.ref_id[k], q.cand[k][m]);
      }
    }
  });
  clk.lap(0);
  FME_TRY(amvp_round_trip(c, ntasks, s));
  clk.lap(1);
  // ---- jobs: one xMotionEstimation per (request, reference), in request order ----
  HIP_TRY(c->h_pi_jobs.reserve((size_t)nj));
  HIP_TRY(c->h_pi_ext.reserve((size_t)nj));
  fme_job* const jobs = c->h_pi_jobs.p;
  fme_tz_ext* const ext = c->h_pi_ext.p;
  std::vector<uint8_t>& amvp_idx = c->pi_amvp_idx;
  amvp_idx.resize((size_t)nj);
  par_for(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; i++) {
      const fme_pu_req& q = reqs[i];
      const double ml = c->mlambda[q.lambda_id];
      for (int k = 0; k < q.num_refs; k++) {
        const int jx = base[i] + k;
        uint32_t best;
        const int idx = task_of[jx] >= 0 ? amvp_pick(tsad + task_of[jx], 2, ml, best) : 0;
        amvp_idx[jx] = (uint8_t)idx;
        const uint32_t bits = blk_bits_p(q.part_size) + ref_bits(k, q.num_refs) + mvp_idx_bits(idx, 2);
        uni_job(c, q, q.ref_id[k], q.cand[k][idx], bits, jobs[jx], ext[jx]);
      }
    }
  });
  // ---- 2. integer searches by m_integerMv2Nx2N dependency level ----
  c->pi_src.resize((size_t)nj);   // job whose post-EMI MV is read
  c->pi_lvl.resize((size_t)nj);
  int last[2 * FME_MAX_REFS];     // last 2Nx2N job of m_integerMv2Nx2N[0][k]
  const int max_level = assign_levels(reqs, n, base.data(), [&](int i, int u) { return u - base[i]; }, c->int_mv_2n, ext,
                                      c->pi_src.data(), c->pi_lvl.data(), last);
  clk.lap(2);
  FME_TRY(tz_levels_device(c, jobs, ext, c->pi_src.data(), c->pi_lvl.data(), nj, max_level, s));
  HIP_TRY(hipStreamSynchronize(s));   // phase boundary (fme_pred_inter_phases)
  clk.lap(3);
  // ---- 3. the sub-pel path over every job in request order (compact results to the host) ----
  HIP_TRY(c->d_res.reserve(nj));
  HIP_TRY(c->d_mv.reserve(nj));
  HIP_TRY(c->h_pi_mv.reserve((size_t)nj));
  HIP_TRY(c->h_pi_last.reserve(FME_MAX_REFS));
  FME_TRY(refine_batch(c, c->d_jobs.p, c->d_res.p, c->d_mv.p, nj, s));
  const fme_mv_result* const r = c->h_pi_mv.p;
  HIP_TRY(hipMemcpyAsync(c->h_pi_mv.p, c->d_mv.p, (size_t)nj * sizeof(fme_mv_result), hipMemcpyDeviceToHost, s));
  // m_integerMv2Nx2N[k] after this call: mv_int of the last 2Nx2N request with a reference k
  for (int k = 0; k < FME_MAX_REFS; k++)
    if (last[k] >= 0)
      HIP_TRY(hipMemcpyAsync(c->h_pi_last.p + k, c->d_res.p + last[k], sizeof(fme_result), hipMemcpyDeviceToHost, s));
  FME_TRY(check_rejected(c, s, "fme_pred_inter_p", "rejected by the refinement batch"));
  clk.lap(4);
  // ---- 4. xCheckBestMVP and the reference choice, per request ----
  par_for(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; i++) {
      const fme_pu_req& q = reqs[i];
      const double ml = c->mlambda[q.lambda_id];
      fme_pu_res& o = res[i];
      o = fme_pu_res{};
      uint32_t best = 0xFFFFFFFFu;
      for (int k = 0; k < q.num_refs; k++) {
        const int jx = base[i] + k;
        const fme_mv_result& rr = r[jx];
        const int mx = rr.mv_x, my = rr.mv_y;
        int idx = amvp_idx[jx];
        uint32_t bits = rr.bits, cost = rr.cost;
        check_best_mvp(ml, q.cand[k], q.n_cand[k], mx, my, idx, bits, cost);
        o.ref_cost[k] = cost; o.ref_bits[k] = bits;
        o.ref_mv[k][0] = (int16_t)mx; o.ref_mv[k][1] = (int16_t)my;
        o.ref_mvp_idx[k] = (uint8_t)idx;
        if (cost < best) {
          best = cost;
          o.cost = cost; o.bits = bits;
          o.mv_x = (int16_t)mx;
          o.mv_y = (int16_t)my;
          o.ref_idx = (uint8_t)k; o.mvp_idx = (uint8_t)idx;
          o.mvp_x = q.cand[k][idx][0]; o.mvp_y = q.cand[k][idx][1];
        }
      }
    }
  });
  for (int k = 0; k < FME_MAX_REFS; k++)
    if (last[k] >= 0) {
      c->int_mv_2n[0][k][0] = c->h_pi_last.p[k].mv_int_x;
      c->int_mv_2n[0][k][1] = c->h_pi_last.p[k].mv_int_y;
    }
  clk.lap(5);
  return FME_OK;
}

}  // extern "C"

// ---- predInterSearch on a B slice (TEncSearch.cpp:3746-4105) ---------------------------------------
namespace {

// One request's progress through the B producer.
struct BPu {
  uint32_t mb[3];
  uint32_t cost[2], bits[2];
  int16_t mv[2][2];
  int ridx[2];
  int mvpi[2][FME_MAX_REFS];
  int16_t mvt[2][FME_MAX_REFS][2];
  uint32_t cost_v1, bits_v1;
  int16_t mv_v1[2];
  int ridx_v1;
  int L;            // list of the current bi-pred iteration
  uint32_t mot[2];  // uiMotBits
  int bi0;          // first bi job of this request in the round's list
  int stage;        // 0 waiting, 1 bi-pred iteration issued, 2 decided, 3 next iteration due
  int last_mode;    // uiLastMode after this request's decision
  // bi-pred iteration state (3871-4022)
  int it, niter;
  int16_t mvbi[2][2];
  int ridxbi[2];
  int mvpibi[2][FME_MAX_REFS];
  uint32_t cost_bi, bits_bi;
  int ps_ref[2];          // m_acYuvPred[l]: the reference and MV list l's stored prediction used
  int16_t ps_mv[2][2];
  int bip_ref, bip_mvp;   // bestBiPRefIdxL1, bestBiPMvpL1 (MvdL1ZeroFlag)
};

// One fme_pred_inter_b call.  (i, l, k) = request, list, reference index; its slot is i * 8 + l * 4 + k.
struct BCall {
  fme_ctx* c;
  const fme_pu_req_b* reqs;
  fme_pu_res_b* res;
  int n, fen;
  std::vector<BPu> st;
  std::vector<int> amvp;         // chosen AMVP index per slot
  std::vector<uint32_t> bipd;    // per slot: *puiDistBiP of list-1 references under MvdL1ZeroFlag (4214-4217)
  std::vector<int> ujob, ubeg;   // uni job per slot (-1: none); first uni job per request
  std::vector<int> ukey;         // l * 4 + k of each uni job
  int nu = 0;
  fme_job* uj = nullptr;         // the uni jobs (pinned), searched after b_uni_refine
  const fme_result* ru = nullptr;   // their records
  int last[2 * FME_MAX_REFS];    // last 2Nx2N uni job per (list, reference)
  uint32_t s_end[12];            // the carried NN state after the uni jobs (what a bi round must leave)
  std::vector<uint32_t> rowst;   // [i][9]: NN_pred's array_e slots and C after request i's uni jobs: its bi jobs' inputs
  std::vector<fme_job> bj;       // one round: the bi jobs, their ext, the key tasks, the requests issued
  std::vector<fme_tz_ext> be;
  std::vector<BiKeyTask> keyt;
  std::vector<int> issued;
  size_t key_total = 0;
};

bool l1_copied(const fme_pu_req_b& q, int l, int k) {
  return l == 1 && (q.flags & FME_PU_FAST_ME_GEN_B) && q.l1_to_l0[k] >= 0;
}

int b_validate(const fme_ctx* c, const fme_pu_req_b* reqs, int n) {
  for (int i = 0; i < n; i++) {
    const fme_pu_req_b& q = reqs[i];
    if (!valid_pu(c, q.org_id, q.x, q.y, q.w, q.h) || q.part_size > FME_PART_nRx2N ||
        q.part_idx >= num_parts(q.part_size) || q.lambda_id >= FME_MAX_LAMBDAS || !c->lambda_set[q.lambda_id] ||
        (q.flags & ~(FME_PU_LOSSLESS | FME_PU_FAST_ME_GEN_B | FME_PU_CLIP_BIPRED | FME_PU_MVD_L1_ZERO)))
      return fail(FME_E_INVALID, "fme_pred_inter_b: request %d invalid (shape %dx%d, part %d/%d)", i, q.w, q.h,
                  q.part_size, q.part_idx);
    if (two_part(q.part_size) && q.part_idx == 1 &&
        (i == 0 || reqs[i - 1].part_idx != 0 || reqs[i - 1].part_size != q.part_size ||
         reqs[i - 1].cu_x != q.cu_x || reqs[i - 1].cu_y != q.cu_y))
      return fail(FME_E_INVALID, "fme_pred_inter_b: request %d (second PU) does not follow its CU's first PU", i);
    for (int l = 0; l < 2; l++) {
      if (q.num_refs[l] < 1 || q.num_refs[l] > FME_MAX_REFS)
        return fail(FME_E_INVALID, "fme_pred_inter_b: request %d list %d: %d references", i, l, q.num_refs[l]);
      for (int k = 0; k < q.num_refs[l]; k++) {
        if (q.n_cand[l][k] < 1 || q.n_cand[l][k] > 2 || !valid_ref(c, q.org_id, q.ref_id[l][k]) ||
            (l == 1 && (q.l1_to_l0[k] < -1 || q.l1_to_l0[k] >= q.num_refs[0])))
          return fail(FME_E_INVALID, "fme_pred_inter_b: request %d list %d reference %d invalid", i, l, k);
      }
    }
  }
  return FME_OK;
}

// f(slot, q, l, k, nc, t) for every (request, list, reference) with AMVP tasks: nc = 2 candidates, or 1
// under MvdL1ZeroFlag on list 1; t: its first task.  Returns the number of tasks.
template <typename F>
int b_for_amvp(const BCall& b, F&& f) {
  int t = 0;
  for (int i = 0; i < b.n; i++) {
    const fme_pu_req_b& q = b.reqs[i];
    for (int l = 0; l < 2; l++)
      for (int k = 0; k < q.num_refs[l]; k++) {
        const int nc = q.n_cand[l][k] >= 2 ? 2 : ((q.flags & FME_PU_MVD_L1_ZERO) && l == 1 ? 1 : 0);
        if (nc) f(i * 8 + l * 4 + k, q, l, k, nc, t);
        t += nc;
      }
  }
  return t;
}

// The uni-pred jobs in call order (pinned): one per (request, list, reference) that list 1 does not
// copy from list 0.  Their bits_in leave out uiMbBits[l], which the decision rounds add.
int b_uni_jobs(BCall& b) {
  fme_ctx* c = b.c;
  const int n = b.n;
  b.ujob.assign((size_t)n * 8, -1);
  b.ubeg.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) {
    b.ubeg[i] = b.nu;
    for (int l = 0; l < 2; l++)
      for (int k = 0; k < b.reqs[i].num_refs[l]; k++)
        if (!l1_copied(b.reqs[i], l, k)) b.ujob[i * 8 + l * 4 + k] = b.nu++;
  }
  b.ubeg[n] = b.nu;
  HIP_TRY(c->h_pi_jobs.reserve((size_t)b.nu));
  HIP_TRY(c->h_pi_ext.reserve((size_t)b.nu));
  b.uj = c->h_pi_jobs.p;
  fme_tz_ext* const ue = c->h_pi_ext.p;
  b.ukey.resize((size_t)b.nu);
  par_for(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; i++) {
      const fme_pu_req_b& q = b.reqs[i];
      for (int l = 0; l < 2; l++)
        for (int k = 0; k < q.num_refs[l]; k++) {
          const int u = b.ujob[i * 8 + l * 4 + k];
          if (u < 0) continue;
          const int idx = b.amvp[i * 8 + l * 4 + k];
          uni_job(c, q, q.ref_id[l][k], q.cand[l][k][idx], ref_bits(k, q.num_refs[l]) + mvp_idx_bits(idx, 2), b.uj[u],
                  ue[u]);
          b.ukey[u] = l * 4 + k;
        }
    }
  });
  return FME_OK;
}

// The uni-pred sub-pel path in call order (full records: the tails are re-priced), the searched
// jobs and their records back on the host, the NN state before and after, and rowst.
int b_uni_refine(BCall& b, hipStream_t s) {
  fme_ctx* c = b.c;
  const int nu = b.nu;
  uint32_t s0[12];
  FME_TRY(fme_nn_get_state(c, s0));
  HIP_TRY(c->d_res.reserve(nu));
  HIP_TRY(c->h_pi_ures.reserve((size_t)nu));
  FME_TRY(refine_batch(c, c->d_jobs.p, c->d_res.p, nullptr, nu, s));
  // the searched uni jobs (the rounds replay them) and their records
  HIP_TRY(hipMemcpyAsync(b.uj, c->d_jobs.p, (size_t)nu * sizeof(fme_job), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(c->h_pi_ures.p, c->d_res.p, (size_t)nu * sizeof(fme_result), hipMemcpyDeviceToHost, s));
  FME_TRY(check_rejected(c, s, "fme_pred_inter_b", "rejected by the refinement batch"));
  b.ru = c->h_pi_ures.p;
  FME_TRY(fme_nn_get_state(c, b.s_end));
  b.rowst.resize((size_t)b.n * 9);
  uint32_t cur[9];
  for (int k = 0; k < 9; k++) cur[k] = s0[k];
  for (int i = 0; i < b.n; i++) {
    for (int u = b.ubeg[i]; u < b.ubeg[i + 1]; u++) {   // every uni job is an EMI job
      for (int k = 0; k < (int)b.ru[u].n_emi && k < 8; k++) cur[k] = b.ru[u].emi[k];
      cur[8] = b.ru[u].c;
    }
    std::memcpy(&b.rowst[(size_t)9 * i], cur, sizeof(cur));
    // a per-call array_e reset (FME_NN_IN_SLOT_RESET nets): a bi call has no pushes of its own
    if (c->cfg.nn_mode == 2 && (c->net.input_flags & FME_NN_IN_SLOT_RESET))
      std::memset(&b.rowst[(size_t)9 * i], 0, 8 * sizeof(uint32_t));
  }
  return FME_OK;
}

// Request i's uni-pred outcome (3780-3868) once uiLastMode is known: every job's tail re-priced
// with uiMbBits, the list-1 copies, xCheckBestMVP, the best reference per list.
void b_uni_phase(BCall& b, int i, int last_mode) {
  const fme_pu_req_b& q = b.reqs[i];
  BPu& p = b.st[i];
  fme_pu_res_b& o = b.res[i];
  o = fme_pu_res_b{};
  const double ml = b.c->mlambda[q.lambda_id];
  blk_bits_b(q.part_size, q.part_idx, last_mode, p.mb);
  p.cost[0] = p.cost[1] = p.cost_v1 = p.bits_v1 = 0xFFFFFFFFu;   // everything else of p is still zero
  uint32_t cost_l0[FME_MAX_REFS] = {}, bits_l0[FME_MAX_REFS] = {};
  uint32_t best_bip = 0xFFFFFFFFu;   // bestBiPDist (3805-3810)
  for (int l = 0; l < 2; l++)
    for (int k = 0; k < q.num_refs[l]; k++) {
      int idx = b.amvp[i * 8 + l * 4 + k];
      if ((q.flags & FME_PU_MVD_L1_ZERO) && l == 1 && b.bipd[i * 8 + 4 + k] < best_bip) {
        best_bip = b.bipd[i * 8 + 4 + k];
        p.bip_ref = k;
        p.bip_mvp = idx;
      }
      uint32_t bits = p.mb[l] + ref_bits(k, q.num_refs[l]) + mvp_idx_bits(idx, 2), cst;
      if (l1_copied(q, l, k)) {   // TEncSearch.cpp:3814-3827
        const int k0 = q.l1_to_l0[k];
        mv_copy(p.mvt[1][k], p.mvt[0][k0]);
        cst = cost_l0[k0] - rd_cost(ml, bits_l0[k0]);
        bits += eg_bits(p.mvt[1][k][0] - q.cand[1][k][idx][0]) + eg_bits(p.mvt[1][k][1] - q.cand[1][k][idx][1]);
        cst += rd_cost(ml, bits);
      } else {
        const int u = b.ujob[i * 8 + l * 4 + k];
        const fme_result& r = b.ru[u];
        p.mvt[l][k][0] = r.mv_x; p.mvt[l][k][1] = r.mv_y;
        cst = tail_cost(ml, r, b.uj[u].bits_in, p.mb[l], 1.0);
        bits = r.bits + p.mb[l];
      }
      check_best_mvp(ml, q.cand[l][k], q.n_cand[l][k], p.mvt[l][k][0], p.mvt[l][k][1], idx, bits, cst);
      p.mvpi[l][k] = idx;
      o.ref_cost[l][k] = cst;
      mv_copy(o.ref_mv[l][k], p.mvt[l][k]);
      o.ref_mvp_idx[l][k] = (uint8_t)idx;
      if (l == 0) {
        cost_l0[k] = cst;
        bits_l0[k] = bits;
      }
      if (cst < p.cost[l]) {
        p.cost[l] = cst;
        p.bits[l] = bits;
        mv_copy(p.mv[l], p.mvt[l][k]);
        p.ridx[l] = k;
      }
      if (l == 1 && cst < p.cost_v1 && q.l1_to_l0[k] < 0) {
        p.cost_v1 = cst;
        p.bits_v1 = bits;
        mv_copy(p.mv_v1, p.mvt[1][k]);
        p.ridx_v1 = k;
      }
    }
  o.bi_list = 0xFF;
  o.bi_cost = 0xFFFFFFFFu;
  o.uni_cost[0] = p.cost[0]; o.uni_bits[0] = p.bits[0];
  o.uni_cost[1] = p.cost_v1; o.uni_bits[1] = p.bits_v1;
}

// The decision (4041-4105); bi-pred outcome already in o.bi_* and mvbi / ridxbi / mvpibi.
void b_decide(BCall& b, int i, const int16_t mvbi[2][2], const int ridxbi[2], const int mvpibi[2][FME_MAX_REFS]) {
  const fme_pu_req_b& q = b.reqs[i];
  BPu& p = b.st[i];
  fme_pu_res_b& o = b.res[i];
  if (o.bi_cost <= p.cost[0] && o.bi_cost <= p.cost_v1) {
    p.last_mode = 2;
    o.inter_dir = 3;
    o.bits = o.bi_bits; o.cost = o.bi_cost;
    for (int l = 0; l < 2; l++) {
      const int k = ridxbi[l], m = mvpibi[l][k];
      o.ref_idx[l] = (uint8_t)k; o.mvp_idx[l] = (uint8_t)m;
      mv_copy(o.mv[l], mvbi[l]);
      mv_copy(o.mvp[l], q.cand[l][k][m]);
    }
  } else if (p.cost[0] <= p.cost_v1) {
    const int k = p.ridx[0], m = p.mvpi[0][k];
    p.last_mode = 0;
    o.inter_dir = 1;
    o.bits = p.bits[0]; o.cost = p.cost[0];
    o.ref_idx[0] = (uint8_t)k; o.mvp_idx[0] = (uint8_t)m;
    mv_copy(o.mv[0], p.mv[0]);
    mv_copy(o.mvp[0], q.cand[0][k][m]);
  } else {
    const int k = p.ridx_v1, m = p.mvpi[1][k];
    p.last_mode = 1;
    o.inter_dir = 2;
    o.bits = p.bits_v1; o.cost = p.cost_v1;
    o.ref_idx[1] = (uint8_t)k; o.mvp_idx[1] = (uint8_t)m;
    mv_copy(o.mv[1], p.mv_v1);
    mv_copy(o.mvp[1], q.cand[1][k][m]);
  }
  p.stage = 2;
}

// bi-pred setup (3871-3916): uiMotBits, and under MvdL1ZeroFlag list 1 at its best predictor
void b_bi_setup(BCall& b, int i) {
  const fme_pu_req_b& q = b.reqs[i];
  BPu& p = b.st[i];
  std::memcpy(p.mvbi, p.mv, sizeof(p.mvbi));
  p.ridxbi[0] = p.ps_ref[0] = p.ridx[0];
  p.ridxbi[1] = p.ps_ref[1] = p.ridx[1];
  std::memcpy(p.mvpibi, p.mvpi, sizeof(p.mvpibi));
  std::memcpy(p.ps_mv, p.mv, sizeof(p.ps_mv));
  p.cost_bi = 0xFFFFFFFFu;
  p.mot[0] = p.bits[0] - p.mb[0];
  if (q.flags & FME_PU_MVD_L1_ZERO) {
    const int kb = p.bip_ref;
    p.mvpibi[1][kb] = p.bip_mvp;
    p.mvbi[1][0] = p.ps_mv[1][0] = p.mvt[1][kb][0] = q.cand[1][kb][p.bip_mvp][0];
    p.mvbi[1][1] = p.ps_mv[1][1] = p.mvt[1][kb][1] = q.cand[1][kb][p.bip_mvp][1];
    p.ridxbi[1] = p.ps_ref[1] = kb;
    p.mot[1] = p.mb[1] + ref_bits(kb, q.num_refs[1]) + mvp_idx_bits(p.bip_mvp, 2);
  } else {
    p.mot[1] = p.bits[1] - p.mb[1];
  }
  p.bits_bi = p.mb[2] + p.mot[0] + p.mot[1];
  p.it = 0;
  p.niter = (b.fen == 1 || b.fen == 2 || (q.flags & FME_PU_MVD_L1_ZERO)) ? 1 : 4;
}

// One iteration's key (the other list's stored prediction, 3946-3952 and 4461-4471) and searches
void b_bi_issue(BCall& b, int i) {
  const fme_pu_req_b& q = b.reqs[i];
  BPu& p = b.st[i];
  const bool l1z = (q.flags & FME_PU_MVD_L1_ZERO) != 0;
  int L = p.it % 2;
  if (b.fen == 1 || b.fen == 2) L = p.cost[0] <= p.cost[1] ? 1 : 0;   // FASTINTERSEARCH_MODE1/2 (3931-3941)
  else if (p.it == 0) L = 0;
  if (p.it == 0 && !l1z) {
    p.ps_ref[1 - L] = p.ridx[1 - L];
    mv_copy(p.ps_mv[1 - L], p.mv[1 - L]);
  }
  if (l1z) L = 0;
  p.L = L;
  const int key_off = (int)b.key_total;
  b.key_total += (size_t)q.w * q.h;
  b.keyt.push_back(BiKeyTask{q.x, q.y, q.w, q.h, q.org_id, q.ref_id[1 - L][p.ps_ref[1 - L]], q.cu_x, q.cu_y,
                             p.ps_mv[1 - L][0], p.ps_mv[1 - L][1], key_off,
                             (q.flags & FME_PU_CLIP_BIPRED) ? 1u : 0u});
  const PicDesc& org = b.c->pics[q.org_id];
  const int brange = q.bipred_range ? q.bipred_range : 4;
  p.bi0 = (int)b.bj.size();
  for (int k = 0; k < q.num_refs[L]; k++) {
    const int m = p.mvpibi[L][k];
    fme_job j;
    fme_tz_ext e;   // xSetSearchRange around cMvTemp[L][k], the last ME result of (L, k) (4486-4490)
    search_job(q, org.width, org.height, q.ref_id[L][k], q.cand[L][k][m], p.mvt[L][k][0], p.mvt[L][k][1], brange,
               FME_JOB_BIPRED | FME_JOB_NN_IN, p.mb[2] + p.mot[1 - L] + ref_bits(k, q.num_refs[L]) + mvp_idx_bits(m, 2), key_off, false,
               j, e);
    b.bj.push_back(j);
    b.be.push_back(e);
  }
  p.stage = 1;
  b.issued.push_back(i);
}

// A round's host half: every request whose uiLastMode is known gets its uni-pred outcome, then its
// decision (isBipredRestriction) or its first bi-pred iteration; requests whose last iteration
// changed something get the next one.  Fills bj / be / keyt / issued.
void b_plan_round(BCall& b) {
  b.bj.clear(); b.be.clear(); b.keyt.clear(); b.issued.clear();
  b.key_total = 0;
  for (int i = 0; i < b.n; i++) {
    const fme_pu_req_b& q = b.reqs[i];
    BPu& p = b.st[i];
    if (p.stage == 3) {
      b_bi_issue(b, i);
      continue;
    }
    if (p.stage != 0) continue;
    const bool dep = two_part(q.part_size) && q.part_idx == 1;
    if (dep && b.st[i - 1].stage != 2) continue;   // uiLastMode not known yet
    b_uni_phase(b, i, dep ? b.st[i - 1].last_mode : 0);
    if (q.cu_w == 8 && (q.w < 8 || q.h < 8)) {   // isBipredRestriction
      b_decide(b, i, p.mv, p.ridx, p.mvpi);
      continue;
    }
    b_bi_setup(b, i);
    b_bi_issue(b, i);
  }
}

// A round's device half: keys, the bi-pred integer searches, the sub-pel path; results in c->h_pi_rs.
int b_run_round(BCall& b, hipStream_t s) {
  fme_ctx* c = b.c;
  FME_TRY(grow_keys(c, b.key_total));
  c->n_keys = b.key_total;
  HIP_TRY(c->d_bikey.reserve(b.keyt.size()));
  HIP_TRY(hipMemcpyAsync(c->d_bikey.p, b.keyt.data(), b.keyt.size() * sizeof(BiKeyTask), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(c->d_key_invalid.p, 0, sizeof(int32_t), s));
  BiKeyArgs ka{c->d_bikey.p, c->d_pics.p, c->d_keys.p, (int32_t)b.keyt.size(), nullptr, (int64_t)b.key_total,
               c->cfg.bit_depth};
  HIP_TRY(launch_bi_key(ka, s));
  // the round's bi jobs alone: in call order each sits right after its request's uni jobs, reads
  // the carried NN state there and writes none (TEncSearch.cpp:88-134), so each is refined as an
  // FME_JOB_NN_IN job whose row is that state (rowst, computed once from the uni records) instead
  // of refining every uni job again around them.  The jobs go up once: the bi-pred integer search
  // (xPatternSearch) writes their MVs in place and the refinement reads them there.
  const int nbj = (int)b.bj.size();
  HIP_TRY(c->h_pi_seq.reserve((size_t)nbj));
  HIP_TRY(c->h_pi_rs.reserve((size_t)nbj));
  HIP_TRY(c->h_pi_rows.reserve((size_t)nbj * 9));
  fme_job* const seq = c->h_pi_seq.p;
  uint32_t* const rows = c->h_pi_rows.p;
  std::memcpy(seq, b.bj.data(), (size_t)nbj * sizeof(fme_job));
  for (int i : b.issued)
    for (int k = 0; k < b.reqs[i].num_refs[b.st[i].L]; k++)
      std::memcpy(rows + (size_t)9 * (b.st[i].bi0 + k), &b.rowst[(size_t)9 * i], 9 * sizeof(uint32_t));
  HIP_TRY(c->d_jobs.reserve(nbj));
  HIP_TRY(c->d_res.reserve(nbj));
  HIP_TRY(c->d_mv.reserve(nbj));
  HIP_TRY(c->d_tz_ext.reserve(nbj));
  HIP_TRY(c->d_tz_sad.reserve(nbj));
  HIP_TRY(c->d_tz_nn_in.reserve((size_t)nbj * 9));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, seq, (size_t)nbj * sizeof(fme_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_tz_ext.p, b.be.data(), (size_t)nbj * sizeof(fme_tz_ext), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_tz_nn_in.p, rows, (size_t)nbj * 9 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  const uint32_t* const keep_in = c->nn_in;
  const int keep_cap = c->nn_in_cap;
  c->nn_in = c->d_tz_nn_in.p;
  c->nn_in_cap = nbj;
  int rc = tz_run(c, c->d_jobs.p, c->d_tz_ext.p, c->d_tz_sad.p, nbj, s, nullptr);
  if (!rc) rc = refine_batch(c, c->d_jobs.p, c->d_res.p, c->d_mv.p, nbj, s);
  c->nn_in = keep_in;
  c->nn_in_cap = keep_cap;
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_pi_rs.p, c->d_mv.p, (size_t)nbj * sizeof(fme_mv_result), hipMemcpyDeviceToHost, s));
  FME_TRY(check_rejected(c, s, "fme_pred_inter_b", "rejected by a bi-pred round"));
  return fme_nn_set_state(c, b.s_end);   // the bi rows wrote the carried state: back to after the uni jobs
}

// A round's results (3960-4022): each issued request's iteration outcome, then its next iteration
// or its decision.
void b_round_results(BCall& b) {
  const fme_mv_result* const rs = b.c->h_pi_rs.p;
  for (const int i : b.issued) {
    const fme_pu_req_b& q = b.reqs[i];
    BPu& p = b.st[i];
    fme_pu_res_b& o = b.res[i];
    const double ml = b.c->mlambda[q.lambda_id];
    const int L = p.L;
    bool changed = false;
    std::memset(o.bi_ref_cost, 0, sizeof(o.bi_ref_cost));
    std::memset(o.bi_ref_mv, 0, sizeof(o.bi_ref_mv));
    for (int k = 0; k < q.num_refs[L]; k++) {
      const fme_mv_result& r = rs[p.bi0 + k];
      p.mvt[L][k][0] = r.mv_x; p.mvt[L][k][1] = r.mv_y;
      uint32_t bits = r.bits, cst = r.cost;
      int idx = p.mvpibi[L][k];
      check_best_mvp(ml, q.cand[L][k], q.n_cand[L][k], r.mv_x, r.mv_y, idx, bits, cst);
      p.mvpibi[L][k] = idx;
      o.bi_ref_cost[k] = cst;
      o.bi_ref_mv[k][0] = r.mv_x; o.bi_ref_mv[k][1] = r.mv_y;
      if (cst < p.cost_bi) {   // 3985-4005
        changed = true;
        p.mvbi[L][0] = r.mv_x; p.mvbi[L][1] = r.mv_y;
        p.ridxbi[L] = k;
        p.cost_bi = cst;
        p.mot[L] = bits - p.mb[2] - p.mot[1 - L];
        p.bits_bi = bits;
        if (p.niter != 1) {   // setAllMv + motionCompensation of list L
          p.ps_ref[L] = k;
          p.ps_mv[L][0] = r.mv_x; p.ps_mv[L][1] = r.mv_y;
        }
      }
    }
    o.bi_list = (uint8_t)L; o.bi_iters = (uint8_t)(p.it + 1);
    if (changed && p.it + 1 < p.niter) {
      p.it++;
      p.stage = 3;
      continue;
    }
    if (!changed && p.cost_bi <= p.cost[0] && p.cost_bi <= p.cost[1]) {   // 4008-4021
      for (int l = 0; l < ((q.flags & FME_PU_MVD_L1_ZERO) ? 1 : 2); l++) {
        const int k = p.ridxbi[l];
        check_best_mvp(ml, q.cand[l][k], q.n_cand[l][k], p.mvbi[l][0], p.mvbi[l][1], p.mvpibi[l][k], p.bits_bi,
                       p.cost_bi);
      }
    }
    o.bi_cost = p.cost_bi; o.bi_bits = p.bits_bi;
    b_decide(b, i, p.mvbi, p.ridxbi, p.mvpibi);
  }
}

}  // namespace

extern "C" {

// The GPU sees:
//   1. one AMVP template-cost launch over every (request, list, reference) with two candidates;
//   2. the uni-pred integer searches by m_integerMv2Nx2N dependency level (per list and reference);
//   3. one fme_refine over the uni-pred jobs in call order.  Their bits_in leave out uiMbBits, which
//      depends on the previous PU's decision (uiLastMode); the searches never read bits_in, so the
//      host re-prices each tail exactly (tail_cost);
//   4. rounds (b_plan_round, b_run_round, b_round_results).  FEN 1/2 and MvdL1ZeroFlag run one bi-pred
//      iteration, FEN 0/3 up to four (each on the key of the other list's current bi-pred best); only
//      the second PU of a two-PU CU waits for a round's decisions, so there are at most 2 x 4 rounds.
int fme_pred_inter_b(fme_ctx* c, const fme_pu_req_b* reqs, fme_pu_res_b* res, int n, void* stream) {
  if (!c || (n > 0 && (!reqs || !res))) return fail(FME_E_INVALID, "fme_pred_inter_b: null argument");
  if (n <= 0) return n == 0 ? FME_OK : fail(FME_E_INVALID, "fme_pred_inter_b: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  PiClock clk(c);
  // ---- validation (nothing runs on a bad batch) ----
  FME_TRY(b_validate(c, reqs, n));
  FME_TRY(sync_tables(c, s));
  BCall b{c, reqs, res, n, c->cfg.fast_inter_mode};
  // ---- 1. xEstimateMvPredAMVP template costs over every (request, list, reference) ----
  b.amvp.assign((size_t)n * 8, 0);
  b.bipd.assign((size_t)n * 8, 0xFFFFFFFFu);
  const int ntasks = b_for_amvp(b, [](int, const fme_pu_req_b&, int, int, int, int) {});
  HIP_TRY(c->h_pi_tasks.reserve((size_t)ntasks));
  HIP_TRY(c->h_pi_tsad.reserve((size_t)ntasks));
  b_for_amvp(b, [&](int, const fme_pu_req_b& q, int l, int k, int nc, int t) {
    for (int m = 0; m < nc; m++) c->h_pi_tasks.p[t + m] = amvp_task(q, q.ref_id[l][k], q.cand[l][k][m]);
  });
  clk.lap(0);
  FME_TRY(amvp_round_trip(c, ntasks, s));
  b_for_amvp(b, [&](int slot, const fme_pu_req_b& q, int, int, int nc, int t) {
    b.amvp[slot] = amvp_pick(c->h_pi_tsad.p + t, nc, c->mlambda[q.lambda_id], b.bipd[slot]);
  });
  clk.lap(1);
  // ---- 2. uni-pred jobs in call order, integer searches by m_integerMv2Nx2N level ----
  FME_TRY(b_uni_jobs(b));
  c->pi_src.resize((size_t)b.nu);
  c->pi_lvl.resize((size_t)b.nu);
  const int max_level = assign_levels(reqs, n, b.ubeg.data(), [&](int, int u) { return b.ukey[u]; }, c->int_mv_2n,
                                      c->h_pi_ext.p, c->pi_src.data(), c->pi_lvl.data(), b.last);
  clk.lap(2);
  FME_TRY(tz_levels_device(c, b.uj, c->h_pi_ext.p, c->pi_src.data(), c->pi_lvl.data(), b.nu, max_level, s));
  HIP_TRY(hipStreamSynchronize(s));   // phase boundary (fme_pred_inter_phases)
  clk.lap(3);
  // ---- 3. the uni-pred sub-pel path in call order ----
  FME_TRY(b_uni_refine(b, s));
  clk.lap(4);
  // ---- 4. rounds of host decisions and bi-pred searches ----
  b.st.resize((size_t)n);   // zeroed: stage 0
  for (;;) {
    b_plan_round(b);
    if (b.issued.empty()) break;
    FME_TRY(b_run_round(b, s));
    b_round_results(b);
  }
  clk.lap(6);
  // ---- m_integerMv2Nx2N: the last 2Nx2N request's post-EMI integer MV per (list, reference) ----
  for (int key = 0; key < 2 * FME_MAX_REFS; key++)
    if (b.last[key] >= 0) {
      c->int_mv_2n[key >> 2][key & 3][0] = b.ru[b.last[key]].mv_int_x;
      c->int_mv_2n[key >> 2][key & 3][1] = b.ru[b.last[key]].mv_int_y;
    }
  return FME_OK;
}

}  // extern "C"
