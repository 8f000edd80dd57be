// fme_merge_host.h — the host arithmetic of fme_merge_estimate (fme_merge.cpp): the requests'
// expansion into prediction-error tasks, xRestrictBipredMergeCand, the merge-index bits, getCost,
// the strict minima and the uiMRGCost < uiMECost choice (TEncSearch.cpp:3625-3653, 3665-3679,
// 4126-4171).  Plain C++ over include/fme_merge.h: no HIP, so a CPU test can include it alone
// (tests/cpp/test_merge_host.cpp).
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/fme_merge.h"

namespace fme {

static_assert(sizeof(fme_pe_task) == 24 && sizeof(fme_merge_cand) == 12 && sizeof(fme_merge_req) == 96 &&
                  sizeof(fme_merge_res) == 72, "fme_merge.h record layouts");

constexpr uint32_t kNoCost = 0xFFFFFFFFu;   // std::numeric_limits<Distortion>::max()

// TComRdCost::getCost (TComRdCost.h:165): only the lambda term is truncated
inline uint32_t merge_rd_cost(double ml, uint32_t bits) { return (uint32_t)((ml * (double)bits) / 65536.0); }

// uiBitsCand (TEncSearch.cpp:3639-3643)
inline uint32_t merge_idx_bits(int idx, int max_num_merge_cand) {
  return (uint32_t)idx + 1u - (idx == max_num_merge_cand - 1 ? 1u : 0u);
}

// TComDataCU::isBipredRestriction (TComDataCU.cpp:2758-2770): an 8x8 CU's PU with a side below 8
inline bool bipred_restricted(int cu_w, int w, int h) { return cu_w == 8 && (w < 8 || h < 8); }

// Candidate k of request q after xRestrictBipredMergeCand (3665-3679): a bi candidate of a
// restricted PU becomes L0-only, its list-1 field (0, 0), reference -1 (here: slot 0, unused).
inline fme_merge_cand merge_cand_restricted(const fme_merge_req& q, int k) {
  fme_merge_cand c = q.cand[k];
  if (c.inter_dir == 3 && bipred_restricted(q.cu_w, q.w, q.h)) c.inter_dir = 1;
  for (int l = 0; l < 2; l++)
    if (!(c.inter_dir & (1u << l))) {
      c.ref_id[l] = 0;
      c.mv[l][0] = c.mv[l][1] = 0;
    }
  c.reserved = 0;
  return c;
}

// Why a request cannot be run (null: it can), apart from the checks of its tasks.
inline const char* merge_req_problem(const fme_merge_req& q) {
  if (q.max_num_merge_cand < 1 || q.max_num_merge_cand > FME_MRG_MAX_CAND) return "max_num_merge_cand";
  if (q.n_cand > FME_MRG_MAX_CAND) return "n_cand";
  if (q.flags & ~(FME_PE_LOSSLESS | FME_MRG_HAS_ME)) return "flags";
  if (q.n_cand == 0 && !(q.flags & FME_MRG_HAS_ME)) return "neither a candidate nor an ME result";
  for (int k = 0; k < q.n_cand; k++)
    if (q.cand[k].inter_dir < 1 || q.cand[k].inter_dir > 3) return "candidate inter_dir";
  if ((q.flags & FME_MRG_HAS_ME) && (q.me_inter_dir < 1 || q.me_inter_dir > 3)) return "me_inter_dir";
  return nullptr;
}

// Tasks of one request: its n_cand candidates in order, then the ME motion (FME_MRG_HAS_ME).
inline int merge_task_count(const fme_merge_req& q) { return q.n_cand + ((q.flags & FME_MRG_HAS_ME) ? 1 : 0); }

inline fme_pe_task merge_task(const fme_merge_req& q, uint8_t inter_dir, const uint8_t ref_id[2], const int16_t mv[2][2]) {
  fme_pe_task t;
  std::memset(&t, 0, sizeof(t));
  t.x = q.x; t.y = q.y; t.w = q.w; t.h = q.h;
  t.org_id = q.org_id;
  t.flags = (uint8_t)((inter_dir & 3u) | (q.flags & FME_PE_LOSSLESS));
  t.cu_x = q.cu_x; t.cu_y = q.cu_y;
  for (int l = 0; l < 2; l++) {
    if (!(inter_dir & (1u << l))) continue;   // the unused list stays zero
    t.ref_id[l] = ref_id[l];
    t.mv[l][0] = mv[l][0];
    t.mv[l][1] = mv[l][1];
  }
  return t;
}

// Writes the request's tasks to out (merge_task_count of them) and returns their number.
inline int merge_expand(const fme_merge_req& q, fme_pe_task* out) {
  int n = 0;
  for (int k = 0; k < q.n_cand; k++) {
    const fme_merge_cand c = merge_cand_restricted(q, k);
    out[n++] = merge_task(q, c.inter_dir, c.ref_id, c.mv);
  }
  if (q.flags & FME_MRG_HAS_ME) out[n++] = merge_task(q, q.me_inter_dir, q.me_ref_id, q.me_mv);
  return n;
}

// TEncSearch.cpp:3627-3653 and 4126-4171 on the request's distortions (dist: in merge_expand's order).
inline void merge_decide(const fme_merge_req& q, const uint32_t* dist, double motion_lambda, fme_merge_res& r) {
  std::memset(&r, 0, sizeof(r));
  for (int k = 0; k < FME_MRG_MAX_CAND; k++) r.cand_dist[k] = r.cand_cost[k] = kNoCost;
  r.merge_cost = kNoCost;
  for (int k = 0; k < q.n_cand; k++) {
    r.cand_dist[k] = dist[k];
    r.cand_cost[k] = dist[k] + merge_rd_cost(motion_lambda, merge_idx_bits(k, q.max_num_merge_cand));
    if (r.cand_cost[k] < r.merge_cost) {
      r.merge_cost = r.cand_cost[k];
      r.merge_idx = (uint8_t)k;
    }
  }
  fme_merge_cand best;
  std::memset(&best, 0, sizeof(best));
  if (r.merge_cost != kNoCost) {
    best = merge_cand_restricted(q, r.merge_idx);
    r.merge_inter_dir = best.inter_dir;
  }
  r.me_dist = r.me_cost = kNoCost;
  if (q.flags & FME_MRG_HAS_ME) {
    r.me_dist = dist[q.n_cand];
    r.me_cost = r.me_dist + merge_rd_cost(motion_lambda, q.me_bits);
  }
  r.use_merge = r.merge_cost < r.me_cost ? 1 : 0;
  if (r.use_merge) {
    r.inter_dir = best.inter_dir;
    r.cost = r.merge_cost;
    for (int l = 0; l < 2; l++) {
      r.ref_id[l] = best.ref_id[l];
      r.mv[l][0] = best.mv[l][0];
      r.mv[l][1] = best.mv[l][1];
    }
  } else {
    r.inter_dir = q.me_inter_dir;
    r.cost = r.me_cost;
    for (int l = 0; l < 2; l++) {
      const bool used = (q.me_inter_dir & (1u << l)) != 0;
      r.ref_id[l] = used ? q.me_ref_id[l] : 0;
      r.mv[l][0] = used ? q.me_mv[l][0] : 0;
      r.mv[l][1] = used ? q.me_mv[l][1] : 0;
    }
  }
}

}  // namespace fme
