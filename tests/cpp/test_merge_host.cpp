// The host arithmetic of fme_merge_estimate (csrc/fme_merge_host.h) against naive transcriptions
// of TEncSearch.cpp:3625-3653, 3665-3679 and 4126-4171.  Stand-alone: built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_merge_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fme_merge_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// HM's objects, as plainly as the source has them
struct MvField {
  int hor = 0, ver = 0, ref = -1;   // TComMvField: refIdx -1 = unused (here: the picture slot)
};
struct Decision {
  bool merge = false;
  unsigned mrgIdx = 0, mrgDir = 0, dir = 0;
  MvField field[2];
  uint32_t mrgCost = 0xFFFFFFFFu, meErr = 0xFFFFFFFFu, meCost = 0xFFFFFFFFu;
  uint32_t candDist[5], candCost[5];
};

uint32_t naive_get_cost(double lambda, uint32_t b) { return (uint32_t)((lambda * b) / 65536.0); }

// xMergeEstimation's loop and the choice of 4126-4171, over given distortions
Decision naive_decide(const fme_merge_req& q, const uint32_t* dist, double lambda) {
  MvField nb[10];
  unsigned char dirs[5] = {0, 0, 0, 0, 0};
  const int num = q.n_cand;
  for (int k = 0; k < num; k++) {
    dirs[k] = q.cand[k].inter_dir;
    for (int l = 0; l < 2; l++)
      if (dirs[k] & (1 << l)) {
        nb[2 * k + l].hor = q.cand[k].mv[l][0];
        nb[2 * k + l].ver = q.cand[k].mv[l][1];
        nb[2 * k + l].ref = q.cand[k].ref_id[l];
      }
  }
  // xRestrictBipredMergeCand / isBipredRestriction (TComDataCU.cpp:2758-2770)
  if (q.cu_w == 8 && (q.w < 8 || q.h < 8))
    for (int k = 0; k < num; k++)
      if (dirs[k] == 3) {
        dirs[k] = 1;
        nb[(k << 1) + 1] = MvField();
      }
  Decision d;
  for (int k = 0; k < 5; k++) d.candDist[k] = d.candCost[k] = 0xFFFFFFFFu;
  MvField mrg[2];
  for (int k = 0; k < num; k++) {
    uint32_t cost = dist[k];
    unsigned bits = k + 1;
    if (k == q.max_num_merge_cand - 1) bits--;
    cost = cost + naive_get_cost(lambda, bits);
    d.candDist[k] = dist[k];
    d.candCost[k] = cost;
    if (cost < d.mrgCost) {
      d.mrgCost = cost;
      mrg[0] = nb[2 * k];
      mrg[1] = nb[2 * k + 1];
      d.mrgDir = dirs[k];
      d.mrgIdx = k;
    }
  }
  MvField me[2];
  unsigned meDir = 0;
  if (q.flags & FME_MRG_HAS_ME) {
    d.meErr = dist[num];
    d.meCost = d.meErr + naive_get_cost(lambda, q.me_bits);
    meDir = q.me_inter_dir;
    for (int l = 0; l < 2; l++)
      if (meDir & (1 << l)) {
        me[l].hor = q.me_mv[l][0];
        me[l].ver = q.me_mv[l][1];
        me[l].ref = q.me_ref_id[l];
      }
  }
  if (d.mrgCost < d.meCost) {
    d.merge = true;
    d.dir = d.mrgDir;
    d.field[0] = mrg[0];
    d.field[1] = mrg[1];
  } else {
    d.dir = meDir;
    d.field[0] = me[0];
    d.field[1] = me[1];
  }
  return d;
}

const int kShapes[][2] = {{8, 4}, {4, 8}, {8, 8}, {16, 4}, {4, 16}, {16, 8}, {8, 16}, {16, 12}, {12, 16}, {16, 16},
                          {32, 8}, {8, 32}, {32, 16}, {16, 32}, {32, 24}, {24, 32}, {32, 32}, {64, 16}, {16, 64},
                          {64, 32}, {32, 64}, {64, 48}, {48, 64}, {64, 64}};

fme_merge_req random_req(std::mt19937& rng) {
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  fme_merge_req q;
  std::memset(&q, 0, sizeof(q));
  const int s = rnd(0, 23);
  q.w = (uint8_t)kShapes[s][0];
  q.h = (uint8_t)kShapes[s][1];
  q.x = (uint16_t)(4 * rnd(0, 30));
  q.y = (uint16_t)(4 * rnd(0, 30));
  const int big = q.w > q.h ? q.w : q.h;
  q.cu_w = (uint8_t)(big <= 8 ? 8 : big <= 16 ? 16 : big <= 32 ? 32 : 64);
  q.cu_x = (uint16_t)(q.x / q.cu_w * q.cu_w);
  q.cu_y = (uint16_t)(q.y / q.cu_w * q.cu_w);
  q.org_id = (uint8_t)rnd(0, 3);
  q.lambda_id = (uint8_t)rnd(0, 3);
  q.n_cand = (uint8_t)rnd(0, 5);
  q.max_num_merge_cand = (uint8_t)rnd(1, 5);
  for (int k = 0; k < q.n_cand; k++) {
    q.cand[k].inter_dir = (uint8_t)rnd(1, 3);
    for (int l = 0; l < 2; l++) {   // the unused list's fields hold junk, as a caller's array may
      q.cand[k].ref_id[l] = (uint8_t)rnd(0, 7);
      q.cand[k].mv[l][0] = (int16_t)rnd(-300, 300);
      q.cand[k].mv[l][1] = (int16_t)rnd(-300, 300);
    }
  }
  if (q.n_cand == 0 || rnd(0, 3)) {
    q.flags |= FME_MRG_HAS_ME;
    q.me_inter_dir = (uint8_t)rnd(1, 3);
    for (int l = 0; l < 2; l++) {
      q.me_ref_id[l] = (uint8_t)rnd(0, 7);
      q.me_mv[l][0] = (int16_t)rnd(-300, 300);
      q.me_mv[l][1] = (int16_t)rnd(-300, 300);
    }
    q.me_bits = (uint32_t)rnd(0, 40);
  }
  if (rnd(0, 4) == 0) q.flags |= FME_PE_LOSSLESS;
  return q;
}

void test_bits_and_cost() {
  for (int m = 1; m <= 5; m++)
    for (int k = 0; k < 5; k++) {
      unsigned bits = k + 1;
      if (k == m - 1) bits--;
      CHECK(fme::merge_idx_bits(k, m) == bits);
      g_cases++;
    }
  std::mt19937 rng(5);
  for (int i = 0; i < 4000; i++) {
    const double lambda = 65536.0 * std::sqrt((double)(rng() % 100000) / 37.0);
    const uint32_t b = rng() % 64;
    CHECK(fme::merge_rd_cost(lambda, b) == naive_get_cost(lambda, b));
    g_cases++;
  }
  const int sides[] = {4, 8, 12, 16, 24, 32, 48, 64};
  for (int cu : {8, 16, 32, 64})
    for (int w : sides)
      for (int h : sides) {
        CHECK(fme::bipred_restricted(cu, w, h) == (cu == 8 && (w < 8 || h < 8)));
        g_cases++;
      }
}

void test_expand_and_decide() {
  std::mt19937 rng(9);
  for (int i = 0; i < 20000; i++) {
    const fme_merge_req q = random_req(rng);
    CHECK(fme::merge_req_problem(q) == nullptr);
    fme_pe_task tasks[6];
    const int n = fme::merge_expand(q, tasks);
    CHECK(n == fme::merge_task_count(q) && n == q.n_cand + ((q.flags & FME_MRG_HAS_ME) ? 1 : 0));
    const bool restricted = q.cu_w == 8 && (q.w < 8 || q.h < 8);
    for (int k = 0; k < n; k++) {
      const fme_pe_task& t = tasks[k];
      CHECK(t.x == q.x && t.y == q.y && t.w == q.w && t.h == q.h && t.cu_x == q.cu_x && t.cu_y == q.cu_y &&
            t.org_id == q.org_id && t.reserved == 0);
      CHECK((t.flags & FME_PE_LOSSLESS) == (q.flags & FME_PE_LOSSLESS));
      const bool me = k == q.n_cand;
      int dir = me ? q.me_inter_dir : q.cand[k].inter_dir;
      if (!me && dir == 3 && restricted) dir = 1;
      CHECK((t.flags & 3) == dir);
      for (int l = 0; l < 2; l++)
        if (dir & (1 << l)) {
          CHECK(t.ref_id[l] == (me ? q.me_ref_id[l] : q.cand[k].ref_id[l]));
          CHECK(t.mv[l][0] == (me ? q.me_mv[l][0] : q.cand[k].mv[l][0]));
          CHECK(t.mv[l][1] == (me ? q.me_mv[l][1] : q.cand[k].mv[l][1]));
        } else {   // the caller's junk in an unused list does not reach the task
          CHECK(t.ref_id[l] == 0 && t.mv[l][0] == 0 && t.mv[l][1] == 0);
        }
    }
    // distortions from a small range, so that equal costs between candidates and against the ME
    // cost are common
    uint32_t dist[6];
    const uint32_t span = (i & 1) ? 6u : 5000u;
    for (int k = 0; k < 6; k++) dist[k] = 100u + rng() % span;
    const double lambda = (i % 3 == 0) ? 65536.0 : 65536.0 * std::sqrt(7.34 + (double)(i % 50));
    fme_merge_res r;
    fme::merge_decide(q, dist, lambda, r);
    const Decision d = naive_decide(q, dist, lambda);
    CHECK(r.use_merge == (d.merge ? 1 : 0));
    CHECK(r.merge_cost == d.mrgCost && r.me_dist == d.meErr && r.me_cost == d.meCost);
    CHECK(r.merge_idx == d.mrgIdx && r.merge_inter_dir == d.mrgDir && r.inter_dir == d.dir);
    CHECK(r.cost == (d.merge ? d.mrgCost : d.meCost));
    for (int k = 0; k < 5; k++) CHECK(r.cand_dist[k] == d.candDist[k] && r.cand_cost[k] == d.candCost[k]);
    for (int l = 0; l < 2; l++) {
      const bool used = d.field[l].ref >= 0;
      CHECK(used == ((d.dir & (1u << l)) != 0));
      CHECK(r.ref_id[l] == (used ? d.field[l].ref : 0));
      CHECK(r.mv[l][0] == (used ? d.field[l].hor : 0) && r.mv[l][1] == (used ? d.field[l].ver : 0));
    }
    if (!(q.flags & FME_MRG_HAS_ME)) CHECK(r.use_merge == 1);   // the AMP merge-only test
    g_cases++;
  }
}

void test_problems() {
  std::mt19937 rng(3);
  fme_merge_req q = random_req(rng);
  q.n_cand = 2;
  q.cand[0].inter_dir = q.cand[1].inter_dir = 1;
  q.max_num_merge_cand = 5;
  q.flags = FME_MRG_HAS_ME;
  q.me_inter_dir = 1;
  CHECK(fme::merge_req_problem(q) == nullptr);
  fme_merge_req b = q;
  b.max_num_merge_cand = 0;
  CHECK(fme::merge_req_problem(b));
  b = q; b.max_num_merge_cand = 6;
  CHECK(fme::merge_req_problem(b));
  b = q; b.n_cand = 6;
  CHECK(fme::merge_req_problem(b));
  b = q; b.flags |= 0x01;
  CHECK(fme::merge_req_problem(b));
  b = q; b.n_cand = 0; b.flags = 0;
  CHECK(fme::merge_req_problem(b));
  b = q; b.cand[1].inter_dir = 0;
  CHECK(fme::merge_req_problem(b));
  b = q; b.cand[1].inter_dir = 4;
  CHECK(fme::merge_req_problem(b));
  b = q; b.me_inter_dir = 0;
  CHECK(fme::merge_req_problem(b));
  b = q; b.flags = 0;   // merge-only with candidates: fine
  CHECK(fme::merge_req_problem(b) == nullptr);
  g_cases += 10;
}

}  // namespace

int main() {
  static_assert(sizeof(fme_pe_task) == 24 && sizeof(fme_merge_cand) == 12 && sizeof(fme_merge_req) == 96 &&
                    sizeof(fme_merge_res) == 72, "fme_merge.h layouts");
  test_bits_and_cost();
  test_expand_and_decide();
  test_problems();
  std::printf("merge host ok: %ld cases\n", g_cases);
  return 0;
}
