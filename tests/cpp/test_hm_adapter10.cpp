// test_hm_adapter10.cpp — GPU test of the C++ adapter (include/fme_hm.hpp) at bit depth 10
// (SearchConfig::bitDepth = 10, the main10 configurations).
//
// The 8-bit driver's frame (tests/cpp/test_hm_adapter.cpp) widened to 10 bits with low-bit noise, so
// that samples above 255 and the two low bits are exercised: Pel and 16-bit picture setters, two CTU
// rows through CtuRowBatcher with bi-pred keys, xPatternSearchFracDIF (the resident server's 10-bit
// instance), NN_pred and one InterSearchP batch, every result bit-exact against the CPU oracle at
// cfg.bit_depth = 10; the error paths of a 10-bit search; and, with --mc10 <dir>, one motion-
// compensation fixture (raw little-endian files written by tests/test_gpu_hm_main10.py from a mc10_*
// golden) through setPictureYuv16 / setPictureYuv(Pel) / add / run16, compared byte for byte.
// Exit status 0 = all equal.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/fme_hm.hpp"
#include "../../oracle/fme_oracle.h"

namespace {

const int W = 416, H = 240, CTU = 64, PAD = 80;
const double kLambda[4] = {7.340, 20.196, 14.797, 20.196};   // LDP QP22
const int kSizes[][2] = {{8, 4}, {4, 8}, {8, 8}, {16, 8}, {8, 16}, {16, 16}, {32, 16}, {16, 32},
                         {32, 32}, {64, 32}, {32, 64}, {64, 64}, {4, 16}, {12, 16}, {16, 4},
                         {16, 12}, {8, 32}, {24, 32}, {32, 8}, {32, 24}, {64, 16}, {48, 64}};
const int kNumSizes = sizeof(kSizes) / sizeof(kSizes[0]);

int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      if (failures < 20) {                \
        fprintf(stderr, "FAIL: " __VA_ARGS__); \
        fprintf(stderr, "\n");            \
      }                                   \
      failures++;                         \
    }                                     \
  } while (0)

// The 8-bit driver's field at 10 bits: four times its amplitude plus noise of its own in the low
// bits, clipped to 0..1023.
std::vector<int16_t> make_picture(int t, uint32_t seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  double a[8], fx[8], fy[8], ph[8];
  for (int i = 0; i < 8; i++) {
    a[i] = 10 + 30 * U(rng);
    fx[i] = 0.01 + 0.19 * U(rng);
    fy[i] = 0.01 + 0.19 * U(rng);
    ph[i] = 6.2831853 * U(rng);
  }
  std::normal_distribution<double> N(0.0, 2.0);
  std::vector<int16_t> p((size_t)W * H);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      double v = 128;
      for (int i = 0; i < 8; i++) v += a[i] * std::sin(fx[i] * (x + 0.37 * t) + fy[i] * (y + 0.21 * t) + ph[i]) / 3;
      v += N(rng);
      p[(size_t)y * W + x] = (int16_t)std::min(1023.0, std::max(0.0, std::round(4.0 * v + (double)(rng() & 3u) - 1.5)));
    }
  return p;
}

int clip_qpel(int v, int pos, int pic) {   // TComDataCU::clipMv (TComDataCU.cpp:2778-2785)
  const int vmax = (pic + 8 - pos - 1) * 4, vmin = (-64 - 8 - pos + 1) * 4;   // (HM shifts; UB on negatives here)
  return std::min(vmax, std::max(vmin, v));
}
int div4_round(int v) { return (v + 2) >> 2; }   // TComMv::divideByPowerOf2 with rounding

void check_rc(int rc) {
  if (rc != FME_OK) throw fme_hm::Error(rc, fme_last_error());
}

bool same(const fme_result& a, const fme_result& b) {
  return a.mv_int_x == b.mv_int_x && a.mv_int_y == b.mv_int_y && a.mv_x == b.mv_x && a.mv_y == b.mv_y &&
         a.half_x == b.half_x && a.half_y == b.half_y && a.qtr_x == b.qtr_x && a.qtr_y == b.qtr_y &&
         a.frac_cost == b.frac_cost && a.cost == b.cost && a.bits == b.bits && a.c == b.c &&
         a.n_emi == b.n_emi && !memcmp(a.emi, b.emi, sizeof(a.emi)) && a.nn_class == b.nn_class &&
         a.status == b.status;
}


template <typename T>
std::vector<T> read_file(const std::string& path) {
  std::vector<T> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw fme_hm::Error(FME_E_INVALID, "cannot open " + path);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)n / sizeof(T));
  const size_t got = fread(v.data(), sizeof(T), v.size(), f);
  fclose(f);
  if (got != v.size() || (size_t)n % sizeof(T)) throw fme_hm::Error(FME_E_INVALID, path + ": short read");
  return v;
}

template <typename F>
int thrown_code(F f) {   // the Error code f() throws, FME_OK when it does not throw
  try {
    f();
  } catch (const fme_hm::Error& e) {
    return e.code();
  }
  return FME_OK;
}

// One mc10_* fixture (raw files: meta = int32 {refs, width, height, jobs, fill}; ref_y/cb/cr and
// pred_y/cb/cr uint16 planes; jobs = fme_mc_job records) through the 10-bit MotionCompensator.
// On a 10-bit search of its own: the fixture's pictures have their own dimensions and ids 0...
int run_mc10(const fme_hm::SearchConfig& cfg10, const std::string& dir) {
  using namespace fme_hm;
  SearchConfig cfg = cfg10;
  cfg.nnMode = 0;
  FracSearch search(cfg);
  const std::vector<int32_t> meta = read_file<int32_t>(dir + "/meta.bin");
  if (meta.size() != 5) throw Error(FME_E_INVALID, "mc10 meta");
  const int refs = meta[0], w = meta[1], h = meta[2], n = meta[3], cw = w / 2, ch = h / 2;
  const uint16_t fill = (uint16_t)meta[4];
  const std::vector<uint16_t> ry = read_file<uint16_t>(dir + "/ref_y.bin"), rcb = read_file<uint16_t>(dir + "/ref_cb.bin"),
                              rcr = read_file<uint16_t>(dir + "/ref_cr.bin");
  const std::vector<uint16_t> py = read_file<uint16_t>(dir + "/pred_y.bin"), pcb = read_file<uint16_t>(dir + "/pred_cb.bin"),
                              pcr = read_file<uint16_t>(dir + "/pred_cr.bin");
  const std::vector<fme_mc_job> jobs = read_file<fme_mc_job>(dir + "/jobs.bin");
  EXPECT((int)jobs.size() == n && ry.size() == (size_t)refs * w * h && rcb.size() == (size_t)refs * cw * ch &&
             rcr.size() == rcb.size() && py.size() == (size_t)w * h && pcb.size() == (size_t)cw * ch && pcr.size() == pcb.size(),
         "mc10 fixture sizes");
  if (failures) return 0;
  MotionCompensator mc(search);
  auto queue = [&] {
    for (const fme_mc_job& j : jobs)
      mc.add(j.x, j.y, j.w, j.h, j.cu_x, j.cu_y, (j.flags & FME_MC_L0) ? j.ref_id[0] : -1, Mv(j.mv[0][0], j.mv[0][1]),
             (j.flags & FME_MC_L1) ? j.ref_id[1] : -1, Mv(j.mv[1][0], j.mv[1][1]));
  };
  for (int pass = 0; pass < 2; pass++) {   // 0: the 16-bit setter, 1: the Pel setter
    for (int r = 0; r < refs; r++) {
      const uint16_t* y = ry.data() + (size_t)r * w * h;
      const uint16_t* cb = rcb.data() + (size_t)r * cw * ch;
      const uint16_t* cr = rcr.data() + (size_t)r * cw * ch;
      if (pass == 0) {
        mc.setPictureYuv16(r, y, w, cb, cr, cw, w, h);
      } else {
        const std::vector<Pel> sy(y, y + (size_t)w * h), scb(cb, cb + (size_t)cw * ch), scr(cr, cr + (size_t)cw * ch);
        mc.setPictureYuv(r, sy.data(), w, scb.data(), scr.data(), cw, w, h);
      }
    }
    queue();
    if (pass == 0) {   // the 8-bit output planes are refused and the queue is kept
      std::vector<uint8_t> y8((size_t)w * h), c8((size_t)cw * ch), d8((size_t)cw * ch);
      EXPECT(thrown_code([&] { mc.run(y8.data(), w, c8.data(), d8.data(), cw, w, h); }) == FME_E_INVALID,
             "MotionCompensator::run (uint8) on a 10-bit search did not throw FME_E_INVALID");
      EXPECT(mc.pending() == n, "the refused run dropped the queue");
      EXPECT(thrown_code([&] { mc.setPictureYuv8(0, y8.data(), w, c8.data(), d8.data(), cw, w, h); }) == FME_E_INVALID,
             "setPictureYuv8 on a 10-bit search did not throw FME_E_INVALID");
    }
    std::vector<uint16_t> gy((size_t)w * h, fill), gcb((size_t)cw * ch, fill), gcr((size_t)cw * ch, fill);
    mc.run16(gy.data(), w, gcb.data(), gcr.data(), cw, w, h);
    EXPECT(mc.pending() == 0, "MotionCompensator queue not cleared");
    EXPECT(gy == py, "mc10 pass %d: luma differs from the fixture", pass);
    EXPECT(gcb == pcb && gcr == pcr, "mc10 pass %d: chroma differs from the fixture", pass);
  }
  return n;
}

}  // namespace

static int run(const char* mc10_dir) {
  using namespace fme_hm;
  std::vector<std::vector<int16_t>> pics;
  for (int i = 0; i < 5; i++) pics.push_back(make_picture(i == 4 ? 0 : 4 - i, 7 + i));
  std::vector<std::vector<uint16_t>> pics16(5);
  int above8 = 0, low = 0;
  for (int i = 0; i < 5; i++) {
    pics16[i].assign(pics[i].begin(), pics[i].end());
    for (uint16_t v : pics16[i]) {
      above8 += v > 255;
      low |= v & 3;
    }
  }
  EXPECT(above8 > W * H && low == 3, "the pictures do not exercise the 10-bit range");

  SearchConfig cfg;
  cfg.qp = 22;
  cfg.maxJobs = 4096;
  cfg.bitDepth = 10;
  FracSearch search(cfg);
  FracSearch search16(cfg);   // the same pictures through setPicture16
  for (int i = 0; i < 5; i++) {
    search.setPicture(i, pics[i].data(), W, W, H);
    search16.setPicture16(i, pics16[i].data(), W, W, H);
  }
  for (int l = 0; l < 4; l++) {
    search.setLambdaSlot(l, kLambda[l]);
    search16.setLambdaSlot(l, kLambda[l]);
  }

  // ---- error paths of a 10-bit search --------------------------------------------------------
  {
    std::vector<int16_t> bad(pics[0]);
    bad[(size_t)17 * W + 5] = 1024;
    EXPECT(thrown_code([&] { search.setPicture(6, bad.data(), W, W, H); }) == FME_E_UNSUPPORTED,
           "setPicture with a sample of 1024 did not throw FME_E_UNSUPPORTED");
    bad[(size_t)17 * W + 5] = -1;
    EXPECT(thrown_code([&] { search.setPicture(6, bad.data(), W, W, H); }) == FME_E_UNSUPPORTED,
           "setPicture with a sample of -1 did not throw FME_E_UNSUPPORTED");
    std::vector<uint8_t> p8((size_t)W * H, 100);
    EXPECT(thrown_code([&] { search.setPicture8(6, p8.data(), W, W, H); }) == FME_E_INVALID,
           "setPicture8 on a 10-bit search did not throw FME_E_INVALID");
    SearchConfig c12 = cfg;
    c12.bitDepth = 12;
    EXPECT(thrown_code([&] { FracSearch s12(c12); }) == FME_E_UNSUPPORTED, "bitDepth 12 did not throw FME_E_UNSUPPORTED");
    SearchConfig c8;
    c8.nnMode = 0;
    FracSearch s8(c8);
    EXPECT(s8.bitDepth() == 8, "SearchConfig's default depth");
    EXPECT(thrown_code([&] { s8.setPicture16(0, pics16[0].data(), W, W, H); }) == FME_E_INVALID,
           "setPicture16 on an 8-bit search did not throw FME_E_INVALID");
    EXPECT(thrown_code([&] { s8.setPicture(0, pics[0].data(), W, W, H); }) == FME_E_UNSUPPORTED,
           "setPicture with 10-bit samples on an 8-bit search did not throw FME_E_UNSUPPORTED");
    MotionCompensator m8(s8);
    std::vector<uint16_t> o16((size_t)W * H);
    EXPECT(thrown_code([&] { m8.run16(o16.data(), W, o16.data(), o16.data(), W / 2, W, H); }) == FME_E_INVALID,
           "run16 on an 8-bit search did not throw FME_E_INVALID");
  }

  // oracle context over the same inputs
  fme_config oc{10, 1, 1, 22, 1, 0};
  std::unique_ptr<orc_ctx> orc(new orc_ctx());
  orc_init(orc.get(), &oc);
  for (int i = 0; i < 5; i++) orc_set_picture16(orc.get(), i, pics16[i].data(), W, W, H);
  for (int l = 0; l < 4; l++) orc_set_lambda(orc.get(), l, kLambda[l]);
  const std::vector<float> wts = loadWeights("", 22);
  orc_load_nn(orc.get(), wts.data());

  // ---- batch path: one row of CTUs at a time ------------------------------------------------
  std::mt19937 rng(1234);
  auto R = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  CtuRowBatcher batcher(search, 2);
  std::vector<CtuRowBatcher::Ticket> tickets;
  std::vector<std::vector<fme_job>> row_jobs;
  std::vector<std::vector<int16_t>> row_keys;
  const int rows = 2, cols = (W + CTU - 1) / CTU;
  for (int ry = 0; ry < rows; ry++) {
    std::vector<fme_job> jobs;
    std::vector<int16_t> keys;   // oracle copy of the row's key blocks
    for (int cx = 0; cx < cols; cx++) {
      for (int k = 0; k < 60; k++) {
        const int* s = kSizes[R(0, kNumSizes - 1)];
        const int w = s[0], h = s[1];
        const int x0 = cx * CTU, y0 = ry * CTU;
        const int x = std::min(W - w, x0 + 4 * R(0, (CTU - w) / 4)), y = std::min(H - h, y0 + 4 * R(0, (CTU - h) / 4));
        fme_job j{};
        j.x = (uint16_t)(x & ~3);
        j.y = (uint16_t)(y & ~3);
        j.w = (uint8_t)w;
        j.h = (uint8_t)h;
        j.org_id = 4;
        j.ref_id = (uint8_t)R(0, 3);
        j.lambda_id = (uint8_t)R(0, 3);
        j.mvp_x = (int16_t)R(-256, 256);
        j.mvp_y = (int16_t)R(-256, 256);
        const int cpx = clip_qpel(j.mvp_x, j.x, W), cpy = clip_qpel(j.mvp_y, j.y, H);
        j.lt_x = (int16_t)div4_round(clip_qpel(cpx - (64 << 2), j.x, W));
        j.rb_x = (int16_t)div4_round(clip_qpel(cpx + (64 << 2), j.x, W));
        j.lt_y = (int16_t)div4_round(clip_qpel(cpy - (64 << 2), j.y, H));
        j.rb_y = (int16_t)div4_round(clip_qpel(cpy + (64 << 2), j.y, H));
        j.mv_x = (int16_t)std::min<int>(j.rb_x, std::max<int>(j.lt_x, R(-64, 64)));
        j.mv_y = (int16_t)std::min<int>(j.rb_y, std::max<int>(j.lt_y, R(-64, 64)));
        j.bits_in = (uint16_t)R(1, 6);
        j.flags = FME_JOB_EMI;
        j.key_offset = -1;
        if (R(0, 5) == 0) {
          // bi-pred: key = 2*org - pred_other, unclipped (TComYuv::removeHighFreq)
          std::vector<int16_t> key((size_t)w * h);
          const std::vector<int16_t>& org = pics[4];
          const std::vector<int16_t>& oth = pics[R(0, 3)];
          const int ox = std::min(W - w, std::max(0, j.x + R(-3, 3))), oy = std::min(H - h, std::max(0, j.y + R(-3, 3)));
          for (int yy = 0; yy < h; yy++)
            for (int xx = 0; xx < w; xx++)
              key[(size_t)yy * w + xx] = (int16_t)(2 * org[(size_t)(j.y + yy) * W + j.x + xx] - oth[(size_t)(oy + yy) * W + ox + xx]);
          batcher.addBiPred(j, key.data(), w);
          j.flags = FME_JOB_BIPRED;
          j.key_offset = (int32_t)keys.size();
          keys.insert(keys.end(), key.begin(), key.end());
        } else {
          batcher.add(j);
        }
        jobs.push_back(j);
      }
    }
    tickets.push_back(batcher.submit());   // row ry runs while row ry+1 is built
    row_jobs.push_back(jobs);
    row_keys.push_back(keys);
  }
  int total = 0;
  for (int ry = 0; ry < rows; ry++) {
    const std::vector<fme_result> got = batcher.wait(tickets[ry]);
    std::vector<fme_result> want(row_jobs[ry].size());
    orc_set_keys(orc.get(), row_keys[ry].data(), row_keys[ry].size());
    EXPECT(orc_refine(orc.get(), row_jobs[ry].data(), want.data(), (int)want.size()) == 0, "oracle row %d", ry);
    EXPECT(got.size() == want.size(), "row %d size", ry);
    for (size_t i = 0; i < got.size() && i < want.size(); i++)
      EXPECT(same(got[i], want[i]), "row %d job %zu (%dx%d): mv %d,%d vs %d,%d cost %u vs %u", ry, i,
             row_jobs[ry][i].w, row_jobs[ry][i].h, got[i].mv_x, got[i].mv_y, want[i].mv_x, want[i].mv_y,
             got[i].cost, want[i].cost);
    total += (int)got.size();
  }


  // ---- setPicture(Pel*) and setPicture16 give identical results: row 0 again on search16 ------
  {
    CtuRowBatcher b16(search16, 1);
    for (const fme_job& j : row_jobs[0]) {
      if (j.flags & FME_JOB_BIPRED)
        b16.addBiPred(j, row_keys[0].data() + j.key_offset, j.w);
      else
        b16.add(j);
    }
    const std::vector<fme_result> got = b16.wait(b16.submit());
    std::vector<fme_result> want(row_jobs[0].size());
    orc_nn_reset(orc.get());
    orc_set_keys(orc.get(), row_keys[0].data(), row_keys[0].size());
    EXPECT(orc_refine(orc.get(), row_jobs[0].data(), want.data(), (int)want.size()) == 0, "oracle row 0 again");
    int bad = 0;
    for (size_t i = 0; i < got.size() && i < want.size(); i++) bad += !same(got[i], want[i]);
    EXPECT(got.size() == want.size() && bad == 0, "setPicture16: %d jobs of row 0 differ", bad);
  }

  // ---- single-PU entry points ---------------------------------------------------------------
  const int PW = W + 2 * PAD;
  std::vector<std::vector<int16_t>> padded(4, std::vector<int16_t>((size_t)PW * (H + 2 * PAD)));
  for (int r = 0; r < 4; r++)
    for (int y = -PAD; y < H + PAD; y++)
      for (int x = -PAD; x < W + PAD; x++)
        padded[r][(size_t)(y + PAD) * PW + x + PAD] =
            pics[r][(size_t)std::min(H - 1, std::max(0, y)) * W + std::min(W - 1, std::max(0, x))];
  int singles = 0;
  for (size_t i = 0; i < row_jobs[1].size(); i += 7) {
    const fme_job& j = row_jobs[1][i];
    if (j.flags & FME_JOB_BIPRED) continue;
    std::vector<int16_t> key((size_t)j.w * j.h);
    for (int yy = 0; yy < j.h; yy++)
      for (int xx = 0; xx < j.w; xx++) key[(size_t)yy * j.w + xx] = pics[4][(size_t)(j.y + yy) * W + j.x + xx];
    search.setLambda(kLambda[j.lambda_id]);
    search.setPredictor(Mv(j.mvp_x, j.mvp_y));
    Mv mvInt(j.mv_x, j.mv_y), mh, mq;
    Distortion cost = 0;
    const int16_t* refY = padded[j.ref_id].data() + (size_t)(j.y + PAD) * PW + j.x + PAD;
    search.xPatternSearchFracDIF(false, key.data(), j.w, j.w, j.h, refY, PW, &mvInt, mh, mq, cost);
    orc_picture p{nullptr, W, W, H, pics16[j.ref_id].data(), 10};
    int8_t oh[2], oq[2];
    uint32_t ocost = 0;
    orc_frac_dif(&p, key.data(), j.w, j.x, j.y, j.w, j.h, j.mv_x, j.mv_y, j.mvp_x, j.mvp_y,
                 65536.0 * std::sqrt(kLambda[j.lambda_id]), 1, oh, oq, &ocost);
    EXPECT(mh.hor == oh[0] && mh.ver == oh[1] && mq.hor == oq[0] && mq.ver == oq[1] && cost == ocost,
           "xPatternSearchFracDIF job %zu: (%d,%d)(%d,%d) %u vs (%d,%d)(%d,%d) %u", i, mh.hor, mh.ver,
           mq.hor, mq.ver, cost, oh[0], oh[1], oq[0], oq[1], ocost);
    singles++;
  }
  for (int k = 0; k < 40; k++) {   // NN_pred is depth-independent: the same net on a 10-bit context
    uint32_t e[8];
    for (uint32_t& v : e) v = (uint32_t)R(0, 200000);
    const uint32_t C = (uint32_t)R(0, 200000);
    const int* s = kSizes[R(0, kNumSizes - 1)];
    int xh, xq, yh, yq;
    const int cls = search.NN_pred(e, C, s[1], s[0], xh, xq, yh, yq);
    EXPECT(cls == orc_nn_forward(wts.data(), e, C, s[1], s[0], nullptr), "NN_pred %d", k);
    EXPECT(2 * xh + xq == cls % 7 - 3 && 2 * yh + yq == cls / 7 - 3, "NN_pred offsets %d", k);
  }

  const int mc_pus = mc10_dir ? run_mc10(cfg, mc10_dir) : 0;

  // ---- InterSearchP: predInterSearch's P-slice PU / reference loop ----------
  int pi_reqs = 0;
  {
    InterSearchP inter(search);
    inter.reset();
    orc_pred_inter_reset(orc.get());
    check_rc(fme_nn_reset_state(search.ctx()));
    orc_nn_reset(orc.get());
    std::mt19937 rq(7);
    auto Q = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rq); };
    std::vector<fme_pu_req> reqs;
    auto add_cu = [&](int x0, int y0, int s, int depth) {
      const int parts[3][2][4] = {{{0, 0, s, s}, {-1, 0, 0, 0}},
                                  {{0, 0, s, s / 2}, {0, s / 2, s, s / 2}},
                                  {{0, 0, s / 2, s}, {s / 2, 0, s / 2, s}}};
      for (int ps = 0; ps < 3; ps++)
        for (int p = 0; p < 2; p++) {
          if (parts[ps][p][0] < 0) continue;
          fme_pu_req q = {};
          q.x = (uint16_t)(x0 + parts[ps][p][0]); q.y = (uint16_t)(y0 + parts[ps][p][1]);
          q.w = (uint8_t)parts[ps][p][2]; q.h = (uint8_t)parts[ps][p][3];
          q.cu_x = (uint16_t)x0; q.cu_y = (uint16_t)y0;
          q.part_size = (uint8_t)ps;   // FME_PART_2Nx2N, _2NxN, _Nx2N
          q.depth = (uint8_t)depth;
          q.org_id = 4; q.num_refs = 4; q.lambda_id = 0; q.search_range = 64;
          for (int k = 0; k < 4; k++) {
            q.ref_id[k] = (uint8_t)k;
            q.n_cand[k] = (uint8_t)(Q(0, 9) == 0 ? 1 : 2);
            for (int m = 0; m < 2; m++) {
              q.cand[k][m][0] = (int16_t)(4 * (k + 1) * 3 + Q(-24, 24));
              q.cand[k][m][1] = (int16_t)(-4 * (k + 1) * 2 + Q(-24, 24));
            }
          }
          reqs.push_back(q);
          inter.add(q);
        }
    };
    for (int cy = 0; cy + CTU <= 2 * CTU; cy += CTU)
      for (int cx = 0; cx + CTU <= W; cx += CTU) {
        add_cu(cx, cy, 64, 0);
        for (int k = 0; k < 4; k++) add_cu(cx + 32 * (k & 1), cy + 32 * (k >> 1), 32, 1);
      }
    pi_reqs = (int)reqs.size();
    EXPECT(inter.pending() == pi_reqs, "InterSearchP queue size");
    const std::vector<fme_pu_res> got = inter.run();
    std::vector<fme_pu_res> want(reqs.size());
    EXPECT(orc_pred_inter_p(orc.get(), reqs.data(), want.data(), (int)reqs.size()) == 0, "orc_pred_inter_p failed");
    int bad = 0;
    for (size_t i = 0; i < reqs.size(); i++) bad += memcmp(&got[i], &want[i], sizeof(fme_pu_res)) != 0;
    EXPECT(bad == 0, "InterSearchP: %d of %d requests differ from orc_pred_inter_p", bad, pi_reqs);
    EXPECT(inter.pending() == 0, "InterSearchP queue not cleared");
  }

  if (failures) {
    fprintf(stderr, "hm adapter main10: %d failure(s)\n", failures);
    return 1;
  }
  printf("hm adapter main10: %d jobs in %d CTU rows, %d single-PU FracDIF calls, 40 NN_pred calls, %d predInterSearch "
         "requests, %d PU motion compensations bit-exact\n", total, rows, singles, pi_reqs, mc_pus);
  printf("hm adapter main10 ok\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    const char* mc10 = nullptr;
    for (int i = 1; i + 1 < argc; i++)
      if (!strcmp(argv[i], "--mc10")) mc10 = argv[i + 1];
    return run(mc10);
  } catch (const fme_hm::Error& e) {
    fprintf(stderr, "hm adapter main10: error %d: %s\n", e.code(), e.what());
    return 2;
  }
}
