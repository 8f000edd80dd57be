// The host arithmetic of the external-predictor path (csrc/fme_extern_host.h) against naive
// definitions: the row -> record rule for every n_emi and both values of `writes`, the class check
// at its edges, the row-MV check at distances 0, 1 and 2 per component and sign, the batch check of
// the host-array form, and the entry points' argument checks.  Stand-alone: built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_extern_host.py.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fme_extern_host.h"

namespace {

long g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

fme_nn_row make_row(int n_emi, int writes) {
  fme_nn_row r;
  std::memset(&r, 0, sizeof(r));
  for (int s = 0; s < 8; s++) r.e[s] = 1000u + 7u * (uint32_t)s;
  r.c = 0xC0FFEEu;
  r.pu_h = 16;
  r.pu_w = 32;
  r.mv_int_x = -37;
  r.mv_int_y = 212;
  r.n_emi = (uint8_t)n_emi;
  r.writes = (uint8_t)writes;
  r.status = FME_RES_NN_STALE;
  return r;
}

void test_layout() {
  CHECK(sizeof(fme_nn_row) == 64);
  CHECK(offsetof(fme_nn_row, e) == 0 && offsetof(fme_nn_row, c) == 32 && offsetof(fme_nn_row, pu_h) == 36);
  CHECK(offsetof(fme_nn_row, pu_w) == 40 && offsetof(fme_nn_row, mv_int_x) == 44 && offsetof(fme_nn_row, mv_int_y) == 46);
  CHECK(offsetof(fme_nn_row, n_emi) == 48 && offsetof(fme_nn_row, writes) == 49 && offsetof(fme_nn_row, status) == 50);
  CHECK(offsetof(fme_nn_row, reserved) == 52);
  CHECK(FME_RES_NN_EXTERN == 0x08u);
  CHECK((FME_RES_NN_EXTERN & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_NN_DIRECT | FME_RES_REJECTED)) == 0);
  g_cases++;
}

void test_row_record() {
  for (int n_emi = 0; n_emi <= 8; n_emi++)
    for (int writes = 0; writes <= 1; writes++) {
      const fme_nn_row r = make_row(n_emi, writes);
      fme_result out;
      std::memset(&out, 0xAB, sizeof(out));
      fme::extern_row_record(r, out);
      fme_result want;
      std::memset(&want, 0, sizeof(want));
      want.mv_int_x = -37;
      want.mv_int_y = 212;
      want.n_emi = (uint8_t)n_emi;
      if (writes) want.c = 0xC0FFEEu;
      for (int s = 0; s < n_emi; s++) want.emi[s] = 1000u + 7u * (uint32_t)s;
      CHECK(std::memcmp(&out, &want, sizeof(out)) == 0);   // every other field 0, the tail of emi[] too
      g_cases++;
    }
  // a count no job can have is clamped, nothing is read past e[7]
  fme_nn_row r = make_row(200, 1);
  fme_result out;
  fme::extern_row_record(r, out);
  CHECK(out.n_emi == 8 && out.emi[7] == 1049u);
  g_cases++;
}

void test_class_check() {
  CHECK(fme::extern_class_ok(0) && fme::extern_class_ok(24) && fme::extern_class_ok(48));
  CHECK(!fme::extern_class_ok(49) && !fme::extern_class_ok(255) && !fme::extern_class_ok(-1));
  int ok = 0;
  for (int c = 0; c < 256; c++) ok += fme::extern_class_ok(c) ? 1 : 0;
  CHECK(ok == fme::kDirectClasses && ok == 49);
  g_cases += 3;   // 48, 49, 255
}

void test_row_mv_check() {
  // distances 0, 1, 2 in each component and sign, around job MVs at the ends of the int16 range too
  const int bases[3][2] = {{5, -9}, {32767, -32768}, {-32768, 32767}};
  for (const auto& b : bases)
    for (int dx = -2; dx <= 2; dx++)
      for (int dy = -2; dy <= 2; dy++) {
        const bool want = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1;
        CHECK(fme::extern_row_mv_ok(b[0] + dx, b[1] + dy, b[0], b[1]) == want);
        g_cases++;
      }
  fme_nn_row r = make_row(8, 1);
  CHECK(fme::extern_row_ok(r, -37, 212) && fme::extern_row_ok(r, -36, 211) && !fme::extern_row_ok(r, -35, 212));
  CHECK(!fme::extern_row_ok(r, -37, 214));
  r.status = FME_RES_REJECTED;   // a row of a rejected inputs batch is nobody's
  CHECK(!fme::extern_row_ok(r, -37, 212));
  g_cases++;
}

void test_first_refused() {
  fme_job jobs[4];
  fme_nn_row rows[4];
  uint8_t cls[4] = {0, 48, 24, 7};
  std::memset(jobs, 0, sizeof(jobs));
  for (int i = 0; i < 4; i++) {
    rows[i] = make_row(8, 1);
    jobs[i].mv_x = (int16_t)(-37 + (i & 1));
    jobs[i].mv_y = (int16_t)(212 - (i >> 1));
  }
  CHECK(fme::extern_first_refused(jobs, rows, cls, 4) == -1);
  CHECK(fme::extern_first_refused(jobs, nullptr, cls, 4) == -1);
  CHECK(fme::extern_first_refused(jobs, rows, cls, 0) == -1);
  cls[2] = 49;
  CHECK(fme::extern_first_refused(jobs, rows, cls, 4) == 2 && fme::extern_first_refused(jobs, nullptr, cls, 4) == 2);
  cls[2] = 24;
  cls[3] = 255;
  CHECK(fme::extern_first_refused(jobs, nullptr, cls, 4) == 3 && fme::extern_first_refused(jobs, nullptr, cls, 3) == -1);
  cls[3] = 7;
  rows[1].mv_int_x = -34;   // two samples from job 1's -36
  CHECK(fme::extern_first_refused(jobs, rows, cls, 4) == 1 && fme::extern_first_refused(jobs, nullptr, cls, 4) == -1);
  g_cases += 6;
}

void test_requests() {
  int ctx = 0, jobs = 0, rows = 0, cls = 0, out = 0;
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, 5, false) == 0);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, 0, false) == 1);
  CHECK(fme::extern_inputs_request(&ctx, nullptr, nullptr, 0, false) == 1);
  CHECK(fme::extern_inputs_request(nullptr, &jobs, &rows, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_inputs_request(&ctx, nullptr, &rows, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, nullptr, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, -1, false) == FME_E_INVALID);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, 5, true) == FME_E_STATE);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, 0, true) == FME_E_STATE);
  CHECK(fme::extern_inputs_request(&ctx, &jobs, &rows, -1, true) == FME_E_INVALID);   // a bad argument comes first
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, &out, 5, false) == 0);
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, &out, 0, false) == 1);
  CHECK(fme::extern_at_request(&ctx, nullptr, nullptr, nullptr, 0, false) == 1);
  CHECK(fme::extern_at_request(nullptr, &jobs, &cls, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_at_request(&ctx, nullptr, &cls, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_at_request(&ctx, &jobs, nullptr, &out, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, nullptr, 5, false) == FME_E_INVALID);
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, &out, -3, false) == FME_E_INVALID);
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, &out, 5, true) == FME_E_STATE);
  CHECK(fme::extern_at_request(&ctx, &jobs, &cls, &out, -3, true) == FME_E_INVALID);
  g_cases += 20;
}

}  // namespace

int main() {
  test_layout();
  test_row_record();
  test_class_check();
  test_row_mv_check();
  test_first_refused();
  test_requests();
  std::printf("extern host ok: %ld cases\n", g_cases);
  return 0;
}
