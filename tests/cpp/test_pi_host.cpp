// test_pi_host.cpp — the predInterSearch producers' host arithmetic, on a CPU.
//
// Includes only csrc/fme_pi_host.h: the bit counts, the search-job builder (xSetSearchRange), the
// AMVP choice, xCheckBestMVP and the m_integerMv2Nx2N dependency levels with their launch order,
// each checked against a definition written out naively here.  Built with
// -fsanitize=address,undefined (tests/test_pi_host.py); every array is a heap block of exactly the
// size the functions are told, so an index past the end is an ASan error.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fme_pi_host.h"

using namespace fme;

// nnfme/synth.py ALL_PU_SIZES
static const int kShapes[][2] = {{8, 4},   {4, 8},   {8, 8},   {8, 16},  {16, 8},  {16, 16}, {32, 16}, {16, 32},
                                 {32, 32}, {64, 32}, {32, 64}, {64, 64}, {4, 16},  {12, 16}, {16, 4},  {16, 12},
                                 {8, 32},  {24, 32}, {32, 8},  {32, 24}, {64, 16}, {64, 48}, {16, 64}, {48, 64}};
static const int kNumShapes = (int)(sizeof(kShapes) / sizeof(kShapes[0]));

static int g_fail = 0, g_cases = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      g_fail++;                          \
    }                                    \
  } while (0)

static uint32_t g_seed = 20240607u;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive

// ---- eg_bits, mvp_idx_bits ---------------------------------------------------------------------
static void test_bits() {
  for (int v = -32768; v <= 32767; v++) {
    const uint32_t t = v <= 0 ? (uint32_t)(-2 * v + 1) : (uint32_t)(2 * v);
    int lg = 0;
    while ((t >> (lg + 1)) != 0) lg++;
    if (eg_bits(v) != (uint32_t)(2 * lg + 1)) {
      CHECK(false, "eg_bits(%d) = %u, expected %d", v, eg_bits(v), 2 * lg + 1);
      return;
    }
  }
  // tests/test_pred_inter.py::test_mvp_idx_bits_table
  CHECK(mvp_idx_bits(0, 2) == 1 && mvp_idx_bits(1, 2) == 1 && mvp_idx_bits(0, 1) == 0, "mvp_idx_bits table");
  const int vs[8] = {0, 1, -1, 2, -2, 3, 7, -8};
  const uint32_t es[8] = {1, 3, 3, 5, 5, 5, 7, 9};
  for (int k = 0; k < 8; k++) CHECK(eg_bits(vs[k]) == es[k], "eg_bits(%d)", vs[k]);
  g_cases += 65536 + 11;
}

// ---- search_job --------------------------------------------------------------------------------
// clipMv's bounds for a CU at cu on a picture axis of length len, full-pel (both are multiples of 4
// in quarter-pel, so round4 of a clipped value lies between them)
static int clip_lo(int cu) { return -64 - 8 - cu + 1; }
static int clip_hi(int len, int cu) { return len + 8 - cu - 1; }
static int clip1(int v, int len, int cu) { return std::min(clip_hi(len, cu) * 4, std::max(clip_lo(cu) * 4, v)); }

template <typename Req>
static void one_search_job(const char* what) {
  const int W = 192, H = 128;
  for (int sh = 0; sh < kNumShapes; sh++) {
    const int w = kShapes[sh][0], h = kShapes[sh][1];
    const int xs[5] = {0, W - w, 0, W - w, ((W - w) / 2) & ~3}, ys[5] = {0, 0, H - h, H - h, ((H - h) / 2) & ~3};
    for (int at = 0; at < 5; at++)
      for (const int range : {0, 4, 64})
        for (int rep = 0; rep < 6; rep++) {
          Req q;
          std::memset(&q, 0, sizeof(q));
          q.x = (uint16_t)xs[at]; q.y = (uint16_t)ys[at]; q.w = (uint8_t)w; q.h = (uint8_t)h;
          q.cu_x = (uint16_t)(xs[at] & ~7); q.cu_y = (uint16_t)(ys[at] & ~7);
          q.org_id = (uint8_t)rnd_in(0, 63);
          q.lambda_id = (uint8_t)rnd_in(0, 63);
          q.flags = (uint8_t)((rep & 1) ? FME_PU_LOSSLESS : 0);
          // predictors and centres from well inside to far outside the picture (quarter-pel)
          const int span = rep < 3 ? 64 : 4000;
          const int16_t pred[2] = {(int16_t)rnd_in(-span, span), (int16_t)rnd_in(-span, span)};
          const bool own_centre = (rep % 3) == 2;   // the bi-pred site: the centre is not the predictor
          const int cx = own_centre ? rnd_in(-span, span) : pred[0], cy = own_centre ? rnd_in(-span, span) : pred[1];
          const uint8_t ref_id = (uint8_t)rnd_in(0, 63);
          const uint32_t jf = own_centre ? FME_JOB_BIPRED : FME_JOB_EMI, bits_in = (uint32_t)rnd_in(0, 60);
          const int32_t key_off = own_centre ? rnd_in(0, 1 << 20) * 4 : -1;
          const bool pred2n = !own_centre && (rep & 2);
          fme_job j;
          fme_tz_ext e;
          std::memset(&j, 0xFF, sizeof(j));
          std::memset(&e, 0xFF, sizeof(e));
          search_job(q, W, H, ref_id, pred, cx, cy, range, jf, bits_in, key_off, pred2n, j, e);
          g_cases++;
          CHECK(j.lt_x <= j.rb_x && j.lt_y <= j.rb_y, "%s %dx%d at %d range %d: lt > rb", what, w, h, at, range);
          CHECK(j.lt_x >= clip_lo(q.cu_x) && j.rb_x <= clip_hi(W, q.cu_x) && j.lt_y >= clip_lo(q.cu_y) &&
                    j.rb_y <= clip_hi(H, q.cu_y),
                "%s %dx%d at %d range %d: a corner outside clipMv's bounds", what, w, h, at, range);
          const int ccx = clip1(cx, W, q.cu_x), ccy = clip1(cy, H, q.cu_y);
          // xSetSearchRange written out: the centre clipped, +- range, both corners clipped, >> 2 rounded
          fme_job x;
          std::memset(&x, 0, sizeof(x));
          x.x = q.x; x.y = q.y; x.w = q.w; x.h = q.h;
          x.org_id = q.org_id; x.ref_id = ref_id;
          x.mvp_x = pred[0]; x.mvp_y = pred[1];
          x.lt_x = (int16_t)round4(clip1(ccx - range * 4, W, q.cu_x));
          x.lt_y = (int16_t)round4(clip1(ccy - range * 4, H, q.cu_y));
          x.rb_x = (int16_t)round4(clip1(ccx + range * 4, W, q.cu_x));
          x.rb_y = (int16_t)round4(clip1(ccy + range * 4, H, q.cu_y));
          x.flags = (uint8_t)(jf | ((rep & 1) ? FME_JOB_LOSSLESS : 0u));
          x.lambda_id = q.lambda_id;
          x.bits_in = (uint16_t)bits_in;
          x.key_offset = key_off;
          fme_tz_ext y;
          std::memset(&y, 0, sizeof(y));
          y.cu_x = q.cu_x; y.cu_y = q.cu_y;
          y.flags = pred2n ? FME_TZ_PRED2NX2N : 0;
          y.search_range = (uint8_t)range;
          // every field not named by the inputs is zero (mv, pred2n, reserved): whole-record equality
          CHECK(std::memcmp(&j, &x, sizeof(j)) == 0, "%s %dx%d at %d range %d: job fields", what, w, h, at, range);
          CHECK(std::memcmp(&e, &y, sizeof(e)) == 0, "%s %dx%d at %d range %d: ext fields", what, w, h, at, range);
          if (range == 0)
            CHECK(j.lt_x == j.rb_x && j.lt_y == j.rb_y && j.lt_x == round4(ccx) && j.lt_y == round4(ccy),
                  "%s %dx%d at %d: range 0 is not the clipped centre", what, w, h, at);
        }
  }
}

// ---- assign_levels + level_order ---------------------------------------------------------------
// kind 0: random; 1: a single request; 2: no request reads (all 2Nx2N at depth 0); 3: one chain (every request
// 2Nx2N and reading)
static void one_stream(int kind) {
  const int n = kind == 1 ? 1 : rnd_in(1, 300);
  std::vector<int> beg((size_t)n + 1, 0), is2n((size_t)n), rd((size_t)n), key;
  std::vector<fme_pu_req> reqs((size_t)n);
  std::vector<fme_job> jobs;
  std::vector<fme_tz_ext> ext;
  for (int i = 0; i < n; i++) {
    beg[i] = (int)key.size();
    is2n[i] = kind >= 2 ? 1 : (rnd() % 5 < 2);
    const bool reads = kind == 3 ? true : (kind == 2 ? false : !(is2n[i] && rnd() % 3 == 0));   // depth 0: no read
    rd[i] = reads;
    std::memset(&reqs[i], 0, sizeof(reqs[i]));
    reqs[i].part_size = (uint8_t)(is2n[i] ? FME_PART_2Nx2N : rnd_in(FME_PART_2NxN, FME_PART_nRx2N));
    reqs[i].depth = (uint8_t)(reads ? rnd_in(is2n[i] ? 1 : 0, 3) : 0);
    CHECK(reads_2n(reqs[i]) == reads, "reads_2n(part %d, depth %d)", reqs[i].part_size, reqs[i].depth);
    const int nk = kind == 3 ? 1 : rnd_in(1, 8);
    int slots[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    for (int a = 0; a < nk && kind != 3; a++) std::swap(slots[a], slots[rnd_in(a, 7)]);   // nk distinct slots
    std::sort(slots, slots + nk);
    const int sh = rnd_in(0, kNumShapes - 1);
    for (int a = 0; a < nk; a++) {
      key.push_back(slots[a]);
      fme_job j;
      std::memset(&j, 0, sizeof(j));
      j.w = (uint8_t)kShapes[sh][0];
      j.h = (uint8_t)kShapes[sh][1];
      jobs.push_back(j);
      fme_tz_ext e;
      std::memset(&e, 0, sizeof(e));
      e.flags = reads ? FME_TZ_PRED2NX2N : 0;   // as search_job sets it
      e.pred2n_x = e.pred2n_y = 0x7777;   // must be overwritten exactly where src < 0
      ext.push_back(e);
    }
  }
  const int nj = (int)key.size();
  beg[n] = nj;
  int16_t carried[2][FME_MAX_REFS][2];
  for (int l = 0; l < 2; l++)
    for (int k = 0; k < FME_MAX_REFS; k++)
      for (int d = 0; d < 2; d++) carried[l][k][d] = (int16_t)rnd_in(-2000, 2000);
  std::vector<int> src((size_t)nj, 12345), lvl((size_t)nj, 12345);
  int last[2 * FME_MAX_REFS];
  const int max_level = assign_levels(
      reqs.data(), n, beg.data(), [&](int, int u) { return key[u]; }, carried, ext.data(), src.data(), lvl.data(), last);
  g_cases++;
  // the naive definition: the source of a reader is the latest earlier 2Nx2N request's job on its slot
  std::vector<int> req_of((size_t)nj);
  for (int i = 0; i < n; i++)
    for (int u = beg[i]; u < beg[i + 1]; u++) req_of[u] = i;
  int seen_max = 0;
  for (int i = 0; i < n; i++) {
    int want_level = 0;
    for (int u = beg[i]; u < beg[i + 1]; u++) {
      int want = -1;
      if (ext[u].flags & FME_TZ_PRED2NX2N)
        for (int p = i - 1; p >= 0 && want < 0; p--)
          if (is2n[p])
            for (int v = beg[p]; v < beg[p + 1]; v++)
              if (key[v] == key[u]) want = v;
      CHECK(src[u] == want, "kind %d: src[%d] = %d, the backward scan finds %d", kind, u, src[u], want);
      if (want >= 0) {
        CHECK(lvl[want] < lvl[u], "kind %d: lvl[src] %d >= lvl[%d] %d", kind, lvl[want], u, lvl[u]);
        want_level = std::max(want_level, lvl[want] + 1);
        CHECK(ext[u].pred2n_x == 0x7777 && ext[u].pred2n_y == 0x7777, "kind %d: pred2n of job %d with a source written", kind, u);
      } else if (ext[u].flags & FME_TZ_PRED2NX2N) {
        CHECK(ext[u].pred2n_x == carried[key[u] >> 2][key[u] & 3][0] && ext[u].pred2n_y == carried[key[u] >> 2][key[u] & 3][1],
              "kind %d: job %d without a source did not get the carried value", kind, u);
      } else {
        CHECK(ext[u].pred2n_x == 0x7777 && ext[u].pred2n_y == 0x7777, "kind %d: pred2n of non-reader %d written", kind, u);
      }
    }
    for (int u = beg[i]; u < beg[i + 1]; u++)
      CHECK(lvl[u] == want_level, "kind %d: lvl[%d] = %d, expected %d", kind, u, lvl[u], want_level);
    seen_max = std::max(seen_max, want_level);
    if (kind == 3) CHECK(lvl[beg[i]] == i, "chain: level %d of request %d", lvl[beg[i]], i);
    if (kind == 2) CHECK(lvl[beg[i]] == 0, "no readers: level %d", lvl[beg[i]]);
  }
  CHECK(max_level == seen_max, "kind %d: max_level %d, expected %d", kind, max_level, seen_max);
  for (int k = 0; k < 2 * FME_MAX_REFS; k++) {
    int want = -1;
    for (int u = 0; u < nj; u++)
      if (is2n[req_of[u]] && key[u] == k) want = u;
    CHECK(last[k] == want, "kind %d: last[%d] = %d, the scan finds %d", kind, k, last[k], want);
  }

  std::vector<int32_t> off, fill, order((size_t)nj, -1), pos((size_t)nj, -1), psrc((size_t)nj, 12345);
  std::vector<int> start, byarea;
  level_order(jobs.data(), lvl.data(), nj, max_level, off, fill, start, byarea, order.data(), pos.data());
  level_psrc(src.data(), order.data(), pos.data(), 0, nj, psrc.data());
  CHECK((int)off.size() == max_level + 2 && off[0] == 0 && off[(size_t)max_level + 1] == nj, "kind %d: off ends", kind);
  for (int l = 0; l <= max_level; l++) CHECK(off[l] <= off[l + 1], "kind %d: off decreases at %d", kind, l);
  std::vector<int> hit((size_t)nj, 0);
  for (int q = 0; q < nj; q++) {
    const int u = order[q];
    if (u < 0 || u >= nj) {
      CHECK(false, "kind %d: order[%d] = %d", kind, q, u);
      return;
    }
    hit[u]++;
    CHECK(pos[u] == q, "kind %d: pos is not order's inverse at %d", kind, q);
    CHECK(off[lvl[u]] <= q && q < off[lvl[u] + 1], "kind %d: job %d of level %d at position %d", kind, u, lvl[u], q);
    if (q > 0 && lvl[order[q - 1]] == lvl[u])
      CHECK((int)jobs[order[q - 1]].w * jobs[order[q - 1]].h >= (int)jobs[u].w * jobs[u].h,
            "kind %d: area increases inside level %d at position %d", kind, lvl[u], q);
    if (src[u] >= 0)
      CHECK(psrc[q] == pos[src[u]] && psrc[q] < off[lvl[u]], "kind %d: psrc[%d] = %d", kind, q, psrc[q]);
    else
      CHECK(psrc[q] == -1, "kind %d: psrc[%d] = %d without a source", kind, q, psrc[q]);
  }
  for (int u = 0; u < nj; u++) CHECK(hit[u] == 1, "kind %d: order is no permutation (job %d x %d)", kind, u, hit[u]);
}

// ---- amvp_pick, check_best_mvp -----------------------------------------------------------------
static uint32_t mvd_bits(const int16_t cand[2][2], int m, int mx, int my) {
  return eg_bits(mx - cand[m][0]) + eg_bits(my - cand[m][1]) + mvp_idx_bits(m, 2);
}
static void test_mvp() {
  for (int rep = 0; rep < 2000; rep++) {
    const double ml = 65536.0 * (0.5 + (double)rnd_in(0, 4000) / 64.0);
    const uint32_t sad[2] = {(uint32_t)rnd_in(0, 5000), (uint32_t)rnd_in(0, 5000)};
    uint32_t best = 0;
    const int idx = amvp_pick(sad, 2, ml, best);
    const uint32_t c0 = template_cost(sad[0], 0, ml), c1 = template_cost(sad[1], 1, ml);
    CHECK(idx == (c1 < c0 ? 1 : 0) && best == std::min(c0, c1), "amvp_pick: %u %u -> %d", c0, c1, idx);   // a tie: the first
    CHECK(amvp_pick(sad, 1, ml, best) == 0 && best == c0, "amvp_pick over one candidate");

    int16_t cand[2][2];
    for (auto& cd : cand)
      for (auto& v : cd) v = (int16_t)rnd_in(-300, 300);
    if (rep % 4 == 0) cand[1][0] = cand[0][0], cand[1][1] = cand[0][1];   // equal candidates: equal bits
    const int mx = rnd_in(-400, 400), my = rnd_in(-400, 400), idx0 = rnd_in(0, 1);
    const uint32_t extra = (uint32_t)rnd_in(0, 12), dist = (uint32_t)rnd_in(0, 100000);
    const uint32_t bits0 = extra + mvd_bits(cand, idx0, mx, my), cost0 = dist + rd_cost(ml, bits0);
    int i1 = idx0;
    uint32_t b1 = bits0, c1n = cost0;
    check_best_mvp(ml, cand, 1, mx, my, i1, b1, c1n);
    CHECK(i1 == idx0 && b1 == bits0 && c1n == cost0, "check_best_mvp with one candidate changed something");
    check_best_mvp(ml, cand, 2, mx, my, i1, b1, c1n);
    CHECK(i1 == 0 || i1 == 1, "check_best_mvp: index %d", i1);
    CHECK(b1 == extra + mvd_bits(cand, i1, mx, my) && b1 <= bits0, "check_best_mvp: bits %u for index %d (from %u)", b1, i1, bits0);
    CHECK(b1 <= extra + mvd_bits(cand, 1 - i1, mx, my), "check_best_mvp: the other candidate is cheaper");
    CHECK(i1 == idx0 || b1 < bits0, "check_best_mvp: moved without a gain");
    CHECK(c1n == dist + rd_cost(ml, b1), "check_best_mvp: cost %u", c1n);
    g_cases += 2;
  }
}

int main() {
  test_bits();
  one_search_job<fme_pu_req>("P");
  one_search_job<fme_pu_req_b>("B");
  for (int kind = 1; kind <= 3; kind++) one_stream(kind);
  for (int rep = 0; rep < 200; rep++) one_stream(0);
  test_mvp();
  if (g_fail) {
    std::printf("pi host: %d failures\n", g_fail);
    return 1;
  }
  std::printf("pi host ok: %d cases\n", g_cases);
  return 0;
}
