// The host arithmetic of the cost surface (csrc/fme_surface_host.h) against naive transcriptions:
// the index <-> offset maps against FME_SURF_INDEX and NN_pred()'s class map, the 24 PU shapes
// against their list, the replay of xPatternRefinement (TEncSearch.cpp:4690-4770) with the offset
// tables written out as the source has them (s_acMvRefineH / s_acMvRefineQ, TEncSearch.cpp:212-236),
// the pick and probe rule and the regret record.  Stand-alone: built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_surface_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fme_surface_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

struct Mv { int x, y; };
const Mv s_acMvRefineH[9] = {{0, 0}, {0, -1}, {0, 1}, {-1, 0}, {1, 0}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}};
const Mv s_acMvRefineQ[9] = {{0, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {1, 1}};

// xPatternRefinement on a surface: baseRefMv in full-pel units of the upsampled plane is (0, 0)
// for the half stage and the half pick for the quarter stage; iFrac 2 / 1; the cost of candidate
// cMvTest = baseRefMv + pcMvRefine[i] * iFrac... read from the surface at its quarter-pel offset.
unsigned naive_refinement(const uint32_t* cost, Mv base, int iFrac, Mv& rcMvFrac, uint32_t& best) {
  unsigned uiDistBest = 0xFFFFFFFFu;   // std::numeric_limits<Distortion>::max()
  unsigned uiDirecBest = 0;
  const Mv* pcMvRefine = iFrac == 2 ? s_acMvRefineH : s_acMvRefineQ;
  for (unsigned i = 0; i < 9; i++) {
    const int qx = 2 * base.x + pcMvRefine[i].x * iFrac, qy = 2 * base.y + pcMvRefine[i].y * iFrac;
    const unsigned uiDist = cost[FME_SURF_INDEX(qx, qy)];
    if (uiDist < uiDistBest) {
      uiDistBest = uiDist;
      uiDirecBest = i;
    }
  }
  rcMvFrac = pcMvRefine[uiDirecBest];
  best = uiDistBest;
  return uiDirecBest;
}

void test_maps() {
  bool seen[FME_SURF_POINTS] = {};
  for (int dy = -3; dy <= 3; dy++)
    for (int dx = -3; dx <= 3; dx++) {
      const int i = fme::surf_index(dx, dy);
      CHECK(i == FME_SURF_INDEX(dx, dy) && i >= 0 && i < FME_SURF_POINTS && !seen[i]);
      seen[i] = true;
      CHECK(fme::surf_dx(i) == dx && fme::surf_dy(i) == dy);
      CHECK(i % 7 - 3 == dx && i / 7 - 3 == dy);   // NN_pred(): offset = (cls % 7 - 3, cls / 7 - 3)
      g_cases++;
    }
  // OUT_CLASS of the training data (TEncSearch.cpp:4576-4578)
  for (int hx = -1; hx <= 1; hx++)
    for (int hy = -1; hy <= 1; hy++)
      for (int qx = -1; qx <= 1; qx++)
        for (int qy = -1; qy <= 1; qy++) {
          const double cls = ((hx * 0.5 + qx * 0.25) + 0.75) * 4 + ((hy * 0.5 + qy * 0.25) + 0.75) * 28;
          CHECK((int)cls == FME_SURF_INDEX(2 * hx + qx, 2 * hy + qy));
          g_cases++;
        }
  for (int k = 0; k < 9; k++) {
    CHECK(fme::surf_refine_x(k) == s_acMvRefineH[k].x && fme::surf_refine_x(k) == s_acMvRefineQ[k].x);
    CHECK(fme::surf_refine_h_y(k) == s_acMvRefineH[k].y && fme::surf_refine_q_y(k) == s_acMvRefineQ[k].y);
    g_cases++;
  }
}

void test_shapes() {
  static const int kShapes[24][2] = {{4, 8}, {8, 4}, {8, 8}, {4, 16}, {16, 4}, {8, 16}, {16, 8}, {12, 16},
                                     {16, 12}, {16, 16}, {8, 32}, {32, 8}, {16, 32}, {32, 16}, {24, 32}, {32, 24},
                                     {32, 32}, {16, 64}, {64, 16}, {32, 64}, {64, 32}, {48, 64}, {64, 48}, {64, 64}};
  int ok = 0;
  for (int w = 0; w < 256; w++)
    for (int h = 0; h < 256; h++) {
      bool listed = false;
      for (const auto& s : kShapes) listed |= s[0] == w && s[1] == h;
      CHECK(fme::surf_shape_ok(w, h) == listed);
      ok += listed;
      g_cases++;
    }
  CHECK(ok == 24);
  for (unsigned p = 0; p < 256; p++) {
    CHECK(fme::surf_probe_ok(p) == (p < 49 || p == FME_SURF_NO_PROBE));
    g_cases++;
  }
}

void test_replay_and_pick(std::mt19937& rng) {
  for (int iter = 0; iter < 20000; iter++) {
    uint32_t cost[FME_SURF_POINTS];
    // few distinct values in most cases: ties in both stages; some cases near UINT_MAX
    const uint32_t span = iter % 3 == 0 ? 3u : iter % 3 == 1 ? 12u : 100000u;
    const uint32_t base = iter % 11 == 0 ? 0xFFFFFFFFu - span : rng() % 1000u;
    for (auto& c : cost) c = base + rng() % (span + 1u);
    Mv h, q;
    uint32_t hc, qc;
    naive_refinement(cost, Mv{0, 0}, 2, h, hc);
    naive_refinement(cost, h, 1, q, qc);
    const fme::SurfReplay r = fme::surf_replay(cost);
    CHECK(r.half_x == h.x && r.half_y == h.y && r.qtr_x == q.x && r.qtr_y == q.y);
    CHECK(r.half_cost == hc && r.frac_cost == qc);
    CHECK(r.frac_cost == cost[FME_SURF_INDEX(2 * h.x + q.x, 2 * h.y + q.y)] && r.frac_cost <= r.half_cost);

    const unsigned p0 = rng() % 49u, p1 = iter % 4 == 0 ? FME_SURF_NO_PROBE : rng() % 49u;
    fme_surface_pick p;
    std::memset(&p, 0xAB, sizeof(p));
    fme::surf_pick(cost, p0, p1, p);
    int first = 0;
    for (int i = 0; i < FME_SURF_POINTS; i++)
      if (cost[i] < cost[first]) first = i;
    CHECK(p.min_idx == first && p.min_cost == cost[first] && p.status == 0);
    for (int i = 0; i < first; i++) CHECK(cost[i] > cost[first]);   // the first of equal minima
    CHECK(p.probe[0] == p0 && p.probe[1] == p1 && p.probe_cost[0] == cost[p0]);
    CHECK(p.probe_cost[1] == (p1 == FME_SURF_NO_PROBE ? 0xFFFFFFFFu : cost[p1]));
    CHECK(p.min_cost <= r.frac_cost);

    const unsigned cls = iter % 5 == 0 ? 255u : p0;
    const fme::SurfRegret g = fme::surf_regret(cost, r.half_x, r.half_y, r.qtr_x, r.qtr_y, cls);
    CHECK(g.search_cost == r.frac_cost && g.min_cost == p.min_cost && g.min_idx == p.min_idx);
    CHECK(g.search_idx == FME_SURF_INDEX(2 * h.x + q.x, 2 * h.y + q.y));
    CHECK(g.class_cost == (cls == 255u ? 0xFFFFFFFFu : cost[cls]));
    g_cases++;
  }
}

// A surface on which the two visiting orders differ: equal costs at (-1, -1) and (-1, 0) around the
// half pick; the Q order meets (-1, -1) first, the H order (-1, 0).
void test_order_tie() {
  uint32_t cost[FME_SURF_POINTS];
  for (auto& c : cost) c = 1000;
  cost[FME_SURF_INDEX(0, 0)] = 500;
  cost[FME_SURF_INDEX(-1, -1)] = 400;
  cost[FME_SURF_INDEX(-1, 0)] = 400;
  const fme::SurfReplay r = fme::surf_replay(cost);
  CHECK(r.half_x == 0 && r.half_y == 0 && r.qtr_x == -1 && r.qtr_y == -1 && r.frac_cost == 400);
  g_cases++;
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  test_maps();
  test_shapes();
  test_replay_and_pick(rng);
  test_order_tie();
  std::printf("surface host ok: %ld cases\n", g_cases);
  return 0;
}
