// The host arithmetic of candidate-set refinement (csrc/fme_among_host.h) against naive definitions:
// the slot check over all 256 values, the list check (every refusal), the pick over a list's costs
// with ties, empties and duplicates, the k-best insertion with equal values against a stable sort,
// the batch check of the host-array form, and the entry points' argument checks.  Stand-alone: built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_among_host.py.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fme_among_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

uint32_t g_seed = 12345u;
uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}

void test_constants() {
  CHECK(FME_AMONG_MAX == 8 && FME_AMONG_EMPTY == 0xFFu && FME_RES_NN_AMONG == 0x10u);
  CHECK((FME_RES_NN_AMONG & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_NN_DIRECT | FME_RES_NN_EXTERN | FME_RES_REJECTED)) == 0);
  CHECK(fme::kAmongNone == 0xFFFFFFFFu);
  for (int k = -1; k <= 10; k++) CHECK(fme::among_k_ok(k) == (k >= 1 && k <= 8));
  g_cases++;
}

void test_slots() {
  int ok = 0, empty = 0;
  for (int v = 0; v < 256; v++) {
    CHECK(fme::among_slot_ok(v) == (v <= 48 || v == 255));
    CHECK(fme::among_slot_empty(v) == (v == 255));
    ok += fme::among_slot_ok(v);
    empty += fme::among_slot_empty(v);
    g_cases++;
  }
  CHECK(ok == 50 && empty == 1);
}

bool naive_list_ok(const uint8_t* s, int k) {
  int classes = 0;
  for (int i = 0; i < k; i++) {
    if (s[i] >= 49 && s[i] != 255) return false;
    if (s[i] != 255) classes++;
  }
  return classes > 0;
}

void test_lists() {
  // every refusal by hand
  const uint8_t good[8] = {0, 48, 255, 24, 24, 255, 7, 1};
  for (int k = 1; k <= 8; k++) CHECK(fme::among_list_ok(good, k));
  const uint8_t all_empty[8] = {255, 255, 255, 255, 255, 255, 255, 255};
  for (int k = 1; k <= 8; k++) CHECK(!fme::among_list_ok(all_empty, k));
  for (int bad : {49, 200, 254})
    for (int pos = 0; pos < 8; pos++) {
      uint8_t l[8];
      std::memcpy(l, good, 8);
      l[pos] = (uint8_t)bad;
      CHECK(!fme::among_list_ok(l, 8));
      CHECK(fme::among_list_ok(l, pos) == (pos > 0));   // the bad slot beyond k is not read as part of the list
      g_cases++;
    }
  const uint8_t one_at_end[8] = {255, 255, 255, 255, 255, 255, 255, 3};
  CHECK(fme::among_list_ok(one_at_end, 8) && !fme::among_list_ok(one_at_end, 7));
  // seeded lists of every k against the naive rule, in a buffer of exactly k bytes
  for (int it = 0; it < 4000; it++) {
    const int k = 1 + (int)(rnd() % 8);
    std::vector<uint8_t> l(k);
    for (int s = 0; s < k; s++) {
      const uint32_t r = rnd() % 10;
      l[s] = r == 0 ? 255 : r == 1 ? (uint8_t)(49 + rnd() % 206) : (uint8_t)(rnd() % 49);
    }
    CHECK(fme::among_list_ok(l.data(), k) == naive_list_ok(l.data(), k));
    g_cases++;
  }
}

int naive_pick(const uint8_t* s, const uint32_t* c, int k) {
  uint64_t best = ~0ull;
  int at = -1;
  for (int i = k - 1; i >= 0; i--)   // from the back with <=: the earliest of the least
    if (s[i] != 255 && (uint64_t)c[i] <= best) {
      best = c[i];
      at = i;
    }
  return at;
}

void test_pick() {
  {
    const uint8_t s[8] = {5, 6, 7, 8, 9, 10, 11, 12};
    const uint32_t c[8] = {9, 4, 4, 7, 4, 100, 3, 3};
    CHECK(fme::among_pick(s, c, 8) == 6 && fme::among_pick(s, c, 6) == 1 && fme::among_pick(s, c, 1) == 0);
    const uint32_t flat[8] = {77, 77, 77, 77, 77, 77, 77, 77};
    for (int k = 1; k <= 8; k++) CHECK(fme::among_pick(s, flat, k) == 0);   // every cost ties: slot 0
  }
  {
    const uint8_t s[8] = {255, 255, 20, 255, 20, 3, 255, 255};   // empties in front, middle, end; a duplicate
    const uint32_t c[8] = {0, 0, 50, 0, 50, 50, 0, 0};           // an empty slot's word is never looked at
    CHECK(fme::among_pick(s, c, 8) == 2 && fme::among_pick(s, c, 2) == -1);
    const uint32_t top[8] = {0, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0xFFFFFFFEu, 0, 0};
    CHECK(fme::among_pick(s, top, 8) == 5 && fme::among_pick(s, top, 5) == 2);   // the largest cost is still a cost
  }
  g_cases += 2;
  for (int it = 0; it < 4000; it++) {
    const int k = 1 + (int)(rnd() % 8);
    std::vector<uint8_t> s(k);
    std::vector<uint32_t> c(k);
    for (int i = 0; i < k; i++) {
      s[i] = rnd() % 4 == 0 ? 255 : (uint8_t)(rnd() % 49);
      c[i] = rnd() % 5;   // few values: ties everywhere
    }
    CHECK(fme::among_pick(s.data(), c.data(), k) == naive_pick(s.data(), c.data(), k));
    g_cases++;
  }
}

void test_insert() {
  for (int it = 0; it < 3000; it++) {
    const int k = 1 + (int)(rnd() % 8);
    const int n = 1 + (int)(rnd() % 49);
    std::vector<float> v(n);
    for (int i = 0; i < n; i++) v[i] = (float)(int)(rnd() % 7) - 3.0f;   // equal values everywhere
    std::vector<float> val(k, -99.0f);
    std::vector<uint8_t> cls(k, 0xEE);
    int filled = 0;
    for (int i = 0; i < n; i++) fme::among_insert(val.data(), cls.data(), k, filled, v[i], i);
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return v[a] > v[b]; });
    CHECK(filled == std::min(n, k));
    for (int q = 0; q < filled; q++) CHECK(cls[q] == order[q] && val[q] == v[order[q]]);
    for (int q = filled; q < k; q++) CHECK(cls[q] == 0xEE);   // untouched beyond what is held
    g_cases++;
  }
  // all equal: index order; strictly increasing: reversed
  float val[8];
  uint8_t cls[8];
  int filled = 0;
  for (int i = 0; i < 49; i++) fme::among_insert(val, cls, 8, filled, 1.5f, i);
  for (int q = 0; q < 8; q++) CHECK(cls[q] == q);
  filled = 0;
  for (int i = 0; i < 49; i++) fme::among_insert(val, cls, 8, filled, (float)i, i);
  for (int q = 0; q < 8; q++) CHECK(cls[q] == 48 - q);
  g_cases += 2;
}

fme_nn_row make_row(int x, int y) {
  fme_nn_row r;
  std::memset(&r, 0, sizeof(r));
  r.mv_int_x = (int16_t)x;
  r.mv_int_y = (int16_t)y;
  return r;
}

void test_first_refused() {
  fme_job jobs[4];
  fme_nn_row rows[4];
  std::memset(jobs, 0, sizeof(jobs));
  for (int i = 0; i < 4; i++) {
    jobs[i].mv_x = (int16_t)(10 + i);
    jobs[i].mv_y = (int16_t)(-5);
    rows[i] = make_row(10 + i + (i & 1), -5 - (i >> 1));
  }
  uint8_t cand[12] = {0, 255, 48, 255, 24, 24, 7, 7, 7, 255, 255, 1};   // k = 3
  CHECK(fme::among_first_refused(jobs, rows, cand, 3, 4) == -1);
  CHECK(fme::among_first_refused(jobs, nullptr, cand, 3, 4) == -1);
  CHECK(fme::among_first_refused(jobs, rows, cand, 3, 0) == -1);
  cand[7] = 49;
  CHECK(fme::among_first_refused(jobs, rows, cand, 3, 4) == 2 && fme::among_first_refused(jobs, nullptr, cand, 3, 2) == -1);
  cand[7] = 7;
  cand[11] = 255;   // job 3: all empty
  CHECK(fme::among_first_refused(jobs, nullptr, cand, 3, 4) == 3);
  cand[11] = 1;
  rows[1].mv_int_x = 14;   // two samples from job 1's 11
  CHECK(fme::among_first_refused(jobs, rows, cand, 3, 4) == 1 && fme::among_first_refused(jobs, nullptr, cand, 3, 4) == -1);
  rows[1].mv_int_x = 12;
  rows[0].status = FME_RES_REJECTED;
  CHECK(fme::among_first_refused(jobs, rows, cand, 3, 4) == 0);
  g_cases += 7;
}

void test_requests() {
  int ctx = 0, jobs = 0, cand = 0, out = 0, rows = 0;
  CHECK(fme::among_request(&ctx, &jobs, &cand, 8, &out, 5, false) == 0);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 1, &out, 0, false) == 1);
  CHECK(fme::among_request(&ctx, nullptr, nullptr, 1, nullptr, 0, false) == 1);
  CHECK(fme::among_request(nullptr, &jobs, &cand, 8, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, nullptr, &cand, 8, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, nullptr, 8, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 8, nullptr, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 0, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 9, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 9, &out, 0, false) == FME_E_INVALID);   // k is checked with n == 0 too
  CHECK(fme::among_request(&ctx, &jobs, &cand, 8, &out, -1, false) == FME_E_INVALID);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 8, &out, 5, true) == FME_E_STATE);
  CHECK(fme::among_request(&ctx, &jobs, &cand, 0, &out, 5, true) == FME_E_INVALID);   // a bad argument comes first
  g_cases += 13;
  CHECK(fme::among_net_state(1, true) == 0 && fme::among_net_state(1, false) == FME_E_STATE);
  CHECK(fme::among_net_state(0, true) == FME_E_STATE && fme::among_net_state(2, true) == FME_E_UNSUPPORTED);
  CHECK(fme::among_rank_request(&ctx, &rows, &cand, 3, 5, 1, true) == 0);
  CHECK(fme::among_rank_request(&ctx, &rows, &cand, 3, 0, 1, true) == 1);
  CHECK(fme::among_rank_request(&ctx, nullptr, &cand, 3, 5, 1, true) == FME_E_INVALID);
  CHECK(fme::among_rank_request(&ctx, &rows, nullptr, 3, 5, 1, true) == FME_E_INVALID);
  CHECK(fme::among_rank_request(&ctx, &rows, &cand, 9, 5, 1, true) == FME_E_INVALID);
  CHECK(fme::among_rank_request(&ctx, &rows, &cand, 3, 5, 0, false) == FME_E_STATE);
  CHECK(fme::among_rank_request(&ctx, &rows, &cand, 3, 5, 2, false) == FME_E_UNSUPPORTED);
  CHECK(fme::among_rank_request(nullptr, &rows, &cand, 3, 5, 2, false) == FME_E_INVALID);
  g_cases += 10;
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 4, 5, false, 1, true) == 0);
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 4, 0, false, 1, true) == 1);
  CHECK(fme::among_topk_request(&ctx, nullptr, &out, 4, 5, false, 1, true) == FME_E_INVALID);
  CHECK(fme::among_topk_request(&ctx, &jobs, nullptr, 4, 5, false, 1, true) == FME_E_INVALID);
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 0, 5, false, 1, true) == FME_E_INVALID);
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 4, 5, true, 1, true) == FME_E_STATE);
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 4, 5, false, 0, false) == FME_E_STATE);
  CHECK(fme::among_topk_request(&ctx, &jobs, &out, 4, 5, false, 2, false) == FME_E_UNSUPPORTED);
  g_cases += 8;
}

}  // namespace

int main() {
  test_constants();
  test_slots();
  test_lists();
  test_pick();
  test_insert();
  test_first_refused();
  test_requests();
  std::printf("among host ok: %ld cases\n", g_cases);
  return 0;
}
