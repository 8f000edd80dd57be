// fme_surface_host.h — the arithmetic around a cost surface (include/fme_surface.h) that needs no
// GPU: the index <-> offset maps, the PU shapes a job may have, the replay of xPatternRefinement's
// two stages (TEncSearch.cpp:4690-4770: the half stage visits s_acMvRefineH's offsets, the quarter
// stage s_acMvRefineQ's, each keeping the first strict minimum), the pick and probe rule, and the
// regret record of one job.  Plain C++ over include/fme_surface.h: no HIP, so a CPU test can include
// it alone (tests/cpp/test_surface_host.cpp); the kernel (fme_surface.hip) includes it too, hence
// FME_SURF_HD.
#pragma once

#include <cstdint>

#include "../../include/fme_surface.h"

#if defined(__HIPCC__)
#define FME_SURF_HD __host__ __device__ inline
#else
#define FME_SURF_HD inline
#endif

namespace fme {

static_assert(sizeof(fme_surface) == 392 && sizeof(fme_surface_pick) == 16, "fme_surface.h record layouts");

constexpr uint32_t kSurfNone = 0xFFFFFFFFu;

// index <-> quarter-pel offset; the index is NN_pred()'s class of the offset
FME_SURF_HD int surf_index(int dx, int dy) { return (dy + 3) * 7 + dx + 3; }
FME_SURF_HD int surf_dx(int idx) { return idx % 7 - 3; }
FME_SURF_HD int surf_dy(int idx) { return idx / 7 - 3; }

// The 24 inter PU shapes (2Nx2N, 2NxN, Nx2N and, from CU 16 on, the four AMP splits of CUs 8..64).
FME_SURF_HD bool surf_shape_ok(int w, int h) {
  const int m = w > h ? w : h, n = w > h ? h : w;
  if (m != 8 && m != 16 && m != 32 && m != 64) return false;
  return n == m || 2 * n == m || (m >= 16 && (4 * n == m || 4 * n == 3 * m));
}

FME_SURF_HD bool surf_probe_ok(unsigned p) { return p < (unsigned)FME_SURF_POINTS || p == FME_SURF_NO_PROBE; }

// xPatternRefinement's visiting orders (TEncSearch.cpp:212-236), offset k of each as (x, y)
FME_SURF_HD int surf_refine_x(int k) { return k < 3 ? 0 : (k & 1) ? -1 : 1; }
FME_SURF_HD int surf_refine_h_y(int k) { return k == 0 ? 0 : k == 1 ? -1 : k == 2 ? 1 : k < 5 ? 0 : k < 7 ? -1 : 1; }
FME_SURF_HD int surf_refine_q_y(int k) { return k == 0 ? 0 : k == 1 ? -1 : k == 2 ? 1 : k < 5 ? -1 : k < 7 ? 0 : 1; }

// The first strict minimum in index order, and the probes' costs.
FME_SURF_HD void surf_pick(const uint32_t* cost, unsigned probe0, unsigned probe1, fme_surface_pick& p) {
  uint32_t best = cost[0];
  int at = 0;
  for (int i = 1; i < FME_SURF_POINTS; i++)
    if (cost[i] < best) {
      best = cost[i];
      at = i;
    }
  p.min_cost = best;
  p.min_idx = (uint8_t)at;
  p.probe[0] = (uint8_t)probe0;
  p.probe[1] = (uint8_t)probe1;
  p.probe_cost[0] = probe0 < (unsigned)FME_SURF_POINTS ? cost[probe0] : kSurfNone;
  p.probe_cost[1] = probe1 < (unsigned)FME_SURF_POINTS ? cost[probe1] : kSurfNone;
  p.status = 0;
}

// What xPatternSearchFracDIF decides on a surface.
struct SurfReplay {
  int8_t half_x, half_y, qtr_x, qtr_y;
  uint32_t half_cost, frac_cost;
};

// One stage: the nine offsets around (bx, by) (quarter-pel units) with step `step`, first strict
// minimum from UINT_MAX (uiDistBest = std::numeric_limits<Distortion>::max()).
inline int surf_stage(const uint32_t* cost, int bx, int by, int step, bool quarter, uint32_t& best) {
  best = kSurfNone;
  int dir = 0;
  for (int k = 0; k < 9; k++) {
    const int x = bx + step * surf_refine_x(k);
    const int y = by + step * (quarter ? surf_refine_q_y(k) : surf_refine_h_y(k));
    const uint32_t c = cost[surf_index(x, y)];
    if (c < best) {
      best = c;
      dir = k;
    }
  }
  return dir;
}

inline SurfReplay surf_replay(const uint32_t* cost) {
  SurfReplay r{};
  const int hd = surf_stage(cost, 0, 0, 2, false, r.half_cost);
  r.half_x = (int8_t)surf_refine_x(hd);
  r.half_y = (int8_t)surf_refine_h_y(hd);
  const int qd = surf_stage(cost, 2 * r.half_x, 2 * r.half_y, 1, true, r.frac_cost);
  r.qtr_x = (int8_t)surf_refine_x(qd);
  r.qtr_y = (int8_t)surf_refine_q_y(qd);
  return r;
}

// The regret record of one job: what the search's pick and a given class cost, against the minimum.
struct SurfRegret {
  uint32_t search_cost;   // cost at (2 half + qtr): equals fme_result.frac_cost
  uint32_t class_cost;    // cost at the class (0xFFFFFFFF: no class, e.g. nn_class 255)
  uint32_t min_cost;
  uint8_t search_idx, min_idx;
};

inline SurfRegret surf_regret(const uint32_t* cost, int half_x, int half_y, int qtr_x, int qtr_y, unsigned cls) {
  SurfRegret g{};
  fme_surface_pick p;
  surf_pick(cost, cls, FME_SURF_NO_PROBE, p);
  g.search_idx = (uint8_t)surf_index(2 * half_x + qtr_x, 2 * half_y + qtr_y);
  g.search_cost = cost[g.search_idx];
  g.class_cost = p.probe_cost[0];
  g.min_cost = p.min_cost;
  g.min_idx = p.min_idx;
  return g;
}

}  // namespace fme
