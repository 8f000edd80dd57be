// The host arithmetic of the NN-direct path (csrc/fme_direct_host.h) against naive definitions: the
// class -> offset map against NN_pred()'s class numbering, the half / quarter split against the
// table of the switch's 49 cases (TEncSearch.cpp:136-193, one row of seven per vertical offset), the
// integer / fraction split against the arithmetic shift and mask xPredInterBlk applies to a
// quarter-pel MV component, the packed half / quarter word against fme_result's bytes, and the
// entry points' argument check.  Stand-alone: built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_direct_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fme_direct_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// {half, quarter} of the seven offsets -3 .. 3 as the switch assigns them, the same in x and in y
const int kSplit[7][2] = {{-1, -1}, {-1, 0}, {0, -1}, {0, 0}, {0, 1}, {1, 0}, {1, 1}};

void test_classes() {
  for (int cls = 0; cls < fme::kDirectClasses; cls++) {
    const int col = cls % 7, row = cls / 7;
    CHECK(fme::direct_dx(cls) == col - 3 && fme::direct_dy(cls) == row - 3);
    const int hx = kSplit[col][0], qx = kSplit[col][1], hy = kSplit[row][0], qy = kSplit[row][1];
    CHECK(fme::direct_half(col - 3) == hx && fme::direct_qtr(col - 3) == qx);
    CHECK(fme::direct_half(row - 3) == hy && fme::direct_qtr(row - 3) == qy);
    CHECK(2 * hx + qx == col - 3 && 2 * hy + qy == row - 3);   // what rcMv gets (TEncSearch.cpp:4590-4591)
    fme_result r;
    std::memset(&r, 0, sizeof(r));
    r.half_x = (int8_t)hx;
    r.half_y = (int8_t)hy;
    r.qtr_x = (int8_t)qx;
    r.qtr_y = (int8_t)qy;
    uint32_t word;
    std::memcpy(&word, &r.half_x, sizeof(word));
    CHECK(word == fme::direct_half_qtr_word(cls));
    g_cases++;
  }
  CHECK(fme::direct_dx(24) == 0 && fme::direct_dy(24) == 0 && fme::direct_half_qtr_word(24) == 0u);
}

void test_position_split() {
  // a quarter-pel MV 4 mv + o predicts at integer (4 mv + o) >> 2 with fraction (4 mv + o) & 3
  for (int mv = -70; mv <= 70; mv++)
    for (int o = -3; o <= 3; o++) {
      const int q = 4 * mv + o;
      CHECK(mv + fme::direct_int(o) == (q >> 2));
      CHECK(fme::direct_frac(o) == (q & 3));
      g_cases++;
    }
}

void test_request() {
  int ctx = 0, jobs = 0, out = 0;
  CHECK(fme::direct_request(&ctx, &jobs, &out, 5, 1) == 0);
  CHECK(fme::direct_request(&ctx, &jobs, &out, 5, 2) == 0);
  CHECK(fme::direct_request(&ctx, &jobs, &out, 0, 1) == 1);        // n == 0: the entry point returns 0
  CHECK(fme::direct_request(&ctx, nullptr, nullptr, 0, 2) == 1);   // and needs no arrays
  CHECK(fme::direct_request(nullptr, &jobs, &out, 5, 1) == FME_E_INVALID);
  CHECK(fme::direct_request(&ctx, nullptr, &out, 5, 1) == FME_E_INVALID);
  CHECK(fme::direct_request(&ctx, &jobs, nullptr, 5, 1) == FME_E_INVALID);
  CHECK(fme::direct_request(&ctx, &jobs, &out, -1, 1) == FME_E_INVALID);
  CHECK(fme::direct_request(nullptr, nullptr, nullptr, 0, 1) == FME_E_INVALID);
  CHECK(fme::direct_request(&ctx, &jobs, &out, 5, 0) == FME_E_STATE);   // nn_mode 0: no class to evaluate
  CHECK(fme::direct_request(&ctx, &jobs, &out, 0, 0) == FME_E_STATE);
  CHECK(fme::direct_request(&ctx, &jobs, &out, -1, 0) == FME_E_INVALID);   // a bad argument comes first
  g_cases += 12;
  CHECK((FME_RES_NN_DIRECT & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_REJECTED)) == 0);
  CHECK(FME_RES_NN_DIRECT == 0x04u);
  g_cases++;
}

}  // namespace

int main() {
  test_classes();
  test_position_split();
  test_request();
  std::printf("direct host ok: %ld cases\n", g_cases);
  return 0;
}
