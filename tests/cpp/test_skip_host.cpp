// The host arithmetic of fme_skip_estimate (csrc/fme_skip_host.h) against naive transcriptions of
// TComRdCost.cpp:57-102 / 327-345, TEncSearch.cpp:5287-5320 and the uiNoResidual == 1 loop of
// TEncCu.cpp:1197-1250.  Stand-alone: built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_skip_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "fme_skip_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

typedef unsigned int Distortion;   // TypeDef.h:239

// HM's objects, as plainly as the source has them
struct RdCost {
  double m_dLambda;
  double m_distortionWeight[3];
  // getDistPart (TComRdCost.cpp:341-349) on a block whose DistFunc result is sse
  Distortion getDistPart(Distortion sse, int compID) const {
    if (compID != 0) return ((Distortion)(m_distortionWeight[compID] * sse));
    return sse;
  }
  // calcRdCost, DF_DEFAULT, COST_STANDARD_LOSSY (TComRdCost.cpp:57-102)
  double calcRdCost(double numBits, double distortion) const {
    double lambda = m_dLambda;
    return distortion + (numBits * lambda);
  }
};

struct Naive {
  int best = -1;
  double bestCost = std::numeric_limits<double>::max();   // MAX_DOUBLE: the fresh best CU's total cost
  Distortion dist[5];
  double cost[5];
};

// The uiNoResidual == 1 iteration over the merge candidates (TEncCu.cpp:1197-1250): a candidate
// whose residual pass found no coefficient is not tried again; xCheckBestMode keeps a candidate only
// when its cost is below the best so far.
Naive naive_skip(const fme_skip_req& q, const fme_skip_params& p, const uint32_t (*sse)[3]) {
  RdCost rd;
  rd.m_dLambda = p.lambda;
  rd.m_distortionWeight[0] = 1.0;
  rd.m_distortionWeight[1] = p.chroma_weight[0];
  rd.m_distortionWeight[2] = p.chroma_weight[1];
  Naive r;
  int at = 0;
  for (unsigned uiMergeCand = 0; uiMergeCand < q.n_cand; ++uiMergeCand) {
    if (!(q.cand_mask & (1u << uiMergeCand))) continue;   // mergeCandBuffer[uiMergeCand] == 1
    Distortion distortion = 0;
    for (int comp = 0; comp < 3; comp++) distortion += rd.getDistPart(sse[at][comp], comp);
    const unsigned uiBits = q.bits[uiMergeCand];
    const double cost = rd.calcRdCost(uiBits, distortion);
    r.dist[uiMergeCand] = distortion;
    r.cost[uiMergeCand] = cost;
    if (cost < r.bestCost) {
      r.bestCost = cost;
      r.best = (int)uiMergeCand;
    }
    at++;
  }
  return r;
}

void test_weighting() {
  // truncation toward zero, never rounding; exact products stay exact
  CHECK(fme::skip_weighted(1.0, 12345u) == 12345u);
  CHECK(fme::skip_weighted(0.5, 7u) == 3u);
  CHECK(fme::skip_weighted(1.2599, 10000u) == 12599u || fme::skip_weighted(1.2599, 10000u) == 12598u);
  CHECK(fme::skip_weighted(1.2599, 10000u) == (uint32_t)(1.2599 * 10000.0));
  CHECK(fme::skip_weighted(0.0, 0xFFFFFFFFu) == 0u);
  // a weight whose product lands within 1e-9 below an integer is truncated to the integer below
  const double w = (3000000.0 - 8e-10) / 3000000.0;   // just below 1
  CHECK(w * 3000000.0 < 3000000.0 && 3000000.0 - w * 3000000.0 < 1e-9);
  CHECK(fme::skip_weighted(w, 3000000u) == 2999999u);
  const double w2 = (1000.0 - 5e-10) / 1000.0;
  CHECK(1000.0 - w2 * 1000.0 < 1e-9 && w2 * 1000.0 < 1000.0);
  CHECK(fme::skip_weighted(w2, 1000u) == 999u);
  // the largest admitted weight on the largest chroma SSE of either depth fits Distortion
  CHECK(fme::skip_weighted(fme::kMaxChromaWeight, 32u * 32u * 255u * 255u) == 64u * 32u * 32u * 255u * 255u);
  CHECK((double)fme::kMaxChromaWeight * (32.0 * 32.0 * (double)((1023 * 1023) >> 4)) < 4294967296.0);
  g_cases += 10;
  std::mt19937_64 rng(5);
  const double ws[4] = {1.0, std::pow(2.0, -1.0 / 3.0), std::pow(2.0, 2.0 / 3.0), 1.2599};
  for (int i = 0; i < 4000; i++) {
    const uint32_t s = (uint32_t)(rng() % 66585601ull);
    const double wt = ws[i & 3];
    RdCost rd{0.0, {1.0, wt, wt}};
    CHECK(fme::skip_weighted(wt, s) == rd.getDistPart(s, 1 + (i & 1)));
    g_cases++;
  }
  // UInt arithmetic: the sum wraps
  fme_skip_params p{1.0, {1.0, 1.0}};
  const uint32_t big[3] = {0xFFFFFFF0u, 0x20u, 0x5u};
  CHECK(fme::skip_distortion(p, big) == 0x15u);
  g_cases++;
}

fme_skip_req random_req(std::mt19937_64& rng) {
  fme_skip_req q;
  std::memset(&q, 0, sizeof(q));
  const int s = 8 << (rng() % 4);
  q.w = q.h = (uint8_t)s;
  q.x = (uint16_t)(s * (rng() % 8));
  q.y = (uint16_t)(s * (rng() % 8));
  q.org_id = (uint8_t)(rng() % 4);
  q.n_cand = (uint8_t)(rng() % 6);
  q.cand_mask = (uint8_t)(rng() % 256);
  for (int k = 0; k < 5; k++) {
    q.cand[k].inter_dir = (uint8_t)(1 + rng() % 3);
    for (int l = 0; l < 2; l++) {
      q.cand[k].ref_id[l] = (uint8_t)(1 + rng() % 5);
      q.cand[k].mv[l][0] = (int16_t)((int)(rng() % 2001) - 1000);
      q.cand[k].mv[l][1] = (int16_t)((int)(rng() % 2001) - 1000);
    }
    q.bits[k] = 1 + (uint32_t)(rng() % 40);
  }
  return q;
}

void test_decisions() {
  std::mt19937_64 rng(6);
  const double ws[4] = {1.0, std::pow(2.0, -1.0 / 3.0), std::pow(2.0, 2.0 / 3.0), 1.2599};
  const double lambdas[6] = {7.340, 20.196, 88.78, 360.16, 1193.1, 0.0};
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < 20000; i++) {
    fme_skip_req q = random_req(rng);
    fme_skip_params p{lambdas[rng() % 6], {ws[rng() % 4], ws[rng() % 4]}};
    uint32_t sse[5][3];
    const bool small = (i % 3) == 0;   // small SSEs: many exact cost ties
    for (auto& s : sse)
      for (auto& v : s) v = small ? (uint32_t)(rng() % 3) : (uint32_t)(rng() % 66585601ull);
    if (i % 4 == 1 && q.n_cand >= 2) {   // the same motion twice with equal bits
      q.cand[q.n_cand - 1] = q.cand[0];
      q.bits[q.n_cand - 1] = q.bits[0];
      q.cand_mask |= (uint8_t)(1u | (1u << (q.n_cand - 1)));
    }
    CHECK(fme::skip_req_problem(q) == nullptr);
    // the expansion: the evaluated candidates in index order, the CU its own clipMv origin
    fme_sse_task tasks[5];
    const int m = fme::skip_expand(q, tasks);
    CHECK(m == fme::skip_task_count(q));
    int at = 0;
    for (int k = 0; k < q.n_cand; k++) {
      if (!(q.cand_mask & (1u << k))) continue;
      const fme_sse_task& t = tasks[at];
      CHECK(t.x == q.x && t.y == q.y && t.w == q.w && t.h == q.h && t.cu_x == q.x && t.cu_y == q.y);
      CHECK(t.org_id == q.org_id && t.flags == q.cand[k].inter_dir && t.reserved == 0);
      for (int l = 0; l < 2; l++) {
        const bool used = (q.cand[k].inter_dir >> l) & 1;
        CHECK(t.ref_id[l] == (used ? q.cand[k].ref_id[l] : 0));
        CHECK(t.mv[l][0] == (used ? q.cand[k].mv[l][0] : 0) && t.mv[l][1] == (used ? q.cand[k].mv[l][1] : 0));
      }
      if (i % 4 == 1 && k == q.n_cand - 1 && q.n_cand >= 2)   // the repeated candidate: the same SSEs
        std::memcpy(sse[at], sse[0], sizeof(sse[0]));
      at++;
    }
    CHECK(at == m);
    fme_skip_res r;
    fme::skip_decide(q, p, sse, r);
    const Naive want = naive_skip(q, p, sse);
    CHECK((want.best < 0) == (r.best == FME_SKIP_NONE));
    if (want.best >= 0) {
      CHECK(r.best == want.best && r.best_cost == want.bestCost);
    } else {
      CHECK(r.best_cost == inf);
    }
    at = 0;
    for (int k = 0; k < 5; k++) {
      const bool ev = k < q.n_cand && (q.cand_mask & (1u << k));
      if (ev) {
        CHECK(r.cand_dist[k] == want.dist[k] && r.cand_cost[k] == want.cost[k]);
        CHECK(std::memcmp(r.cand_sse[k], sse[at], sizeof(sse[at])) == 0);
        CHECK(r.cand_cost[k] >= r.best_cost);
        if (k < r.best) CHECK(r.cand_cost[k] > r.best_cost);   // the first with the strictly least cost
        at++;
      } else {
        CHECK(r.cand_dist[k] == 0xFFFFFFFFu && r.cand_cost[k] == inf);
        CHECK(r.cand_sse[k][0] == 0xFFFFFFFFu && r.cand_sse[k][1] == 0xFFFFFFFFu && r.cand_sse[k][2] == 0xFFFFFFFFu);
      }
    }
    for (int k = 0; k < 7; k++) CHECK(r.reserved[k] == 0);
    g_cases++;
  }
}

void test_validity() {
  std::mt19937_64 rng(7);
  fme_skip_req q = random_req(rng);
  q.n_cand = 3;
  q.cand_mask = 7;
  CHECK(fme::skip_req_problem(q) == nullptr);
  fme_skip_req b = q;
  b.n_cand = 6;
  CHECK(fme::skip_req_problem(b) != nullptr);
  b = q;
  b.flags = 1;
  CHECK(fme::skip_req_problem(b) != nullptr);
  b = q;
  b.cand[1].inter_dir = 0;
  CHECK(fme::skip_req_problem(b) != nullptr);
  b.cand_mask = 5;   // the bad candidate is masked out
  CHECK(fme::skip_req_problem(b) == nullptr);
  b = q;
  b.cand[4].inter_dir = 7;   // beyond n_cand: not looked at
  b.cand_mask = 0xFF;
  CHECK(fme::skip_req_problem(b) == nullptr && fme::skip_task_count(b) == 3);
  b = q;
  b.n_cand = 0;
  CHECK(fme::skip_req_problem(b) == nullptr && fme::skip_task_count(b) == 0);
  fme_skip_params p{10.0, {1.0, 1.0}};
  CHECK(fme::skip_params_problem(p) == nullptr);
  p.lambda = -1.0;
  CHECK(fme::skip_params_problem(p) != nullptr);
  p.lambda = std::numeric_limits<double>::quiet_NaN();
  CHECK(fme::skip_params_problem(p) != nullptr);
  p.lambda = 1.0;
  p.chroma_weight[1] = 65.0;
  CHECK(fme::skip_params_problem(p) != nullptr);
  p.chroma_weight[1] = -0.5;
  CHECK(fme::skip_params_problem(p) != nullptr);
  g_cases += 12;
}

}  // namespace

int main() {
  test_weighting();
  test_decisions();
  test_validity();
  std::printf("skip host ok: %ld cases\n", g_cases);
  return 0;
}
