// fme_skip_host.h — the host arithmetic of fme_skip_estimate (fme_skip.cpp): the requests'
// expansion into SSE tasks, the chroma weighting with its truncation (TComRdCost.cpp:343), the CU's
// distortion in UInt arithmetic, calcRdCost (57-102, DF_DEFAULT, COST_STANDARD_LOSSY) and
// xCheckBestMode's strict minimum over the masked-in candidates (TEncCu.cpp:1231-1239).  Plain C++
// over include/fme_skip.h: no HIP, so a CPU test can include it alone
// (tests/cpp/test_skip_host.cpp).  Built with -ffp-contract=off: distortion + bits * lambda is a
// rounded product and a rounded sum, as in the reference's build.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/fme_skip.h"

namespace fme {

static_assert(sizeof(fme_sse_task) == 24 && sizeof(fme_skip_params) == 24 && sizeof(fme_skip_req) == 96 &&
                  sizeof(fme_skip_res) == 136, "fme_skip.h record layouts");

constexpr uint32_t kNoSse = 0xFFFFFFFFu;
constexpr double kMaxChromaWeight = 64.0;   // 32 * 32 * 1023^2 >> 4 and 32 * 32 * 255^2, times 64, stay below 2^32

// getDistPart's chroma branch (TComRdCost.cpp:343): (Distortion)(m_distortionWeight[compID] * sse)
inline uint32_t skip_weighted(double weight, uint32_t sse) { return (uint32_t)(weight * (double)sse); }

// TEncSearch.cpp:5294-5303: distortion = Y + Cb' + Cr', Distortion (UInt) arithmetic
inline uint32_t skip_distortion(const fme_skip_params& p, const uint32_t sse[3]) {
  return sse[0] + skip_weighted(p.chroma_weight[0], sse[1]) + skip_weighted(p.chroma_weight[1], sse[2]);
}

// calcRdCost(bits, distortion), DF_DEFAULT in COST_STANDARD_LOSSY (TComRdCost.cpp:99)
inline double skip_rd_cost(double lambda, uint32_t bits, uint32_t distortion) {
  return (double)distortion + ((double)bits * lambda);
}

inline const char* skip_params_problem(const fme_skip_params& p) {
  if (!std::isfinite(p.lambda) || p.lambda < 0.0) return "lambda";
  for (int c = 0; c < 2; c++)
    if (!std::isfinite(p.chroma_weight[c]) || p.chroma_weight[c] < 0.0 || p.chroma_weight[c] > kMaxChromaWeight)
      return "chroma_weight";
  return nullptr;
}

// The candidates of q that are evaluated, as a mask below 1 << n_cand.
inline unsigned skip_eval_mask(const fme_skip_req& q) { return q.cand_mask & ((1u << q.n_cand) - 1u); }

// Why a request cannot be run (null: it can), apart from the checks of its tasks.
inline const char* skip_req_problem(const fme_skip_req& q) {
  if (q.n_cand > FME_MRG_MAX_CAND) return "n_cand";
  if (q.flags) return "flags";
  const unsigned m = skip_eval_mask(q);
  for (int k = 0; k < q.n_cand; k++)
    if (((m >> k) & 1u) && (q.cand[k].inter_dir < 1 || q.cand[k].inter_dir > 3)) return "candidate inter_dir";
  return nullptr;
}

// Tasks of one request: its evaluated candidates in index order.
inline int skip_task_count(const fme_skip_req& q) { return __builtin_popcount(skip_eval_mask(q)); }

// Writes the request's tasks to out (skip_task_count of them) and returns their number.
inline int skip_expand(const fme_skip_req& q, fme_sse_task* out) {
  const unsigned m = skip_eval_mask(q);
  int n = 0;
  for (int k = 0; k < q.n_cand; k++) {
    if (!((m >> k) & 1u)) continue;
    const fme_merge_cand& c = q.cand[k];
    fme_sse_task t;
    std::memset(&t, 0, sizeof(t));
    t.x = q.x; t.y = q.y; t.w = q.w; t.h = q.h;
    t.org_id = q.org_id;
    t.flags = (uint8_t)(c.inter_dir & 3u);
    t.cu_x = q.x; t.cu_y = q.y;   // a 2Nx2N PU: the CU is its own clipMv origin
    for (int l = 0; l < 2; l++) {
      if (!(c.inter_dir & (1u << l))) continue;   // the unused list stays zero
      t.ref_id[l] = c.ref_id[l];
      t.mv[l][0] = c.mv[l][0];
      t.mv[l][1] = c.mv[l][1];
    }
    out[n++] = t;
  }
  return n;
}

// Steps 3-5 on the request's SSEs (sse: in skip_expand's order).
inline void skip_decide(const fme_skip_req& q, const fme_skip_params& p, const uint32_t (*sse)[3], fme_skip_res& r) {
  std::memset(&r, 0, sizeof(r));
  const double inf = std::numeric_limits<double>::infinity();
  r.best = FME_SKIP_NONE;
  r.best_cost = inf;
  const unsigned m = skip_eval_mask(q);
  int at = 0;
  for (int k = 0; k < FME_MRG_MAX_CAND; k++) {
    if (!((m >> k) & 1u)) {
      r.cand_cost[k] = inf;
      r.cand_dist[k] = r.cand_sse[k][0] = r.cand_sse[k][1] = r.cand_sse[k][2] = kNoSse;
      continue;
    }
    for (int c = 0; c < 3; c++) r.cand_sse[k][c] = sse[at][c];
    r.cand_dist[k] = skip_distortion(p, sse[at]);
    r.cand_cost[k] = skip_rd_cost(p.lambda, q.bits[k], r.cand_dist[k]);
    if (r.cand_cost[k] < r.best_cost) {   // xCheckBestMode: strictly below the best so far
      r.best_cost = r.cand_cost[k];
      r.best = (uint8_t)k;
    }
    at++;
  }
}

}  // namespace fme
