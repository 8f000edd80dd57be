// test_srv_pack.cpp — the single-call server's mailbox, host against kernel, on a CPU.
//
// Includes only csrc/fme_srv_pack.h: packs a FracDIF request with srv_pack_frac (what
// fme_frac_dif_single does), then unpacks it with the block-count and word-mapping functions the
// resident kernel uses (srv_frac_need, srv_put_block, srv_win_loads / srv_key_loads), for every PU
// shape at both bit depths.  Built with -fsanitize=address,undefined (tests/test_srv_pack.py): the
// reference plane has exactly the 4 samples of margin the window needs on each side, so a
// one-sample over-read is an ASan error.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fme_srv_pack.h"

using namespace fme;

// nnfme/synth.py ALL_PU_SIZES
static const int kShapes[][2] = {{8, 4},   {4, 8},   {8, 8},   {8, 16},  {16, 8},  {16, 16}, {32, 16}, {16, 32},
                                 {32, 32}, {64, 32}, {32, 64}, {64, 64}, {4, 16},  {12, 16}, {16, 4},  {16, 12},
                                 {8, 32},  {24, 32}, {32, 8},  {32, 24}, {64, 16}, {64, 48}, {16, 64}, {48, 64}};

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      g_fail++;                          \
    }                                    \
  } while (0)

static uint32_t rnd(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}

static void one(int w, int h, int bd, uint32_t seq) {
  const int bps = srv_bps(bd), pw = w + 8, ph = h + 8, maxv = (1 << bd) - 1;
  uint32_t s = (uint32_t)(w * 131 + h * 7 + bd);
  // the reference plane: exactly the window, the PU origin at (4, 4); samples below 0 and above the
  // range so that the clamp is exercised
  std::vector<int16_t> plane((size_t)pw * ph);
  for (auto& v : plane) v = (int16_t)((int)(rnd(s) % (uint32_t)(maxv + 41)) - 20);
  const int16_t* ref = plane.data() + 4 * pw + 4;   // mv_int = (0, 0)
  const int ks = w + 5;
  std::vector<int16_t> key((size_t)ks * (h - 1) + w);   // no row padding after the last row
  for (auto& v : key) v = (int16_t)((int)(rnd(s) % 3070u) - 1023);
  std::unique_ptr<SrvBox> box(new SrvBox());
  std::memset(box.get(), 0, sizeof(SrvBox));
  const double ml = 12345.678 + w;
  srv_pack_frac(box.get(), seq, bd, (w & 8) != 0, false, key.data(), ks, w, h, ref, pw, 0, 0, -3, 5, ml);

  // the kernel's side: the shape word, the block count, the unpacking
  const uint32_t shape = box->req[0][1];
  CHECK((shape & 3u) == (uint32_t)kSrvFrac, "%dx%d bd %d: kind", w, h, bd);
  CHECK((int)((shape >> 8) & 0xFFu) + 1 == w && (int)((shape >> 16) & 0xFFu) + 1 == h, "%dx%d bd %d: shape", w, h, bd);
  CHECK(((shape & kSrvSad) != 0) == ((w & 8) != 0), "%dx%d bd %d: sad bit", w, h, bd);
  const bool tagged = (shape & kSrvTagged) != 0;
  CHECK(tagged == srv_fits_tagged(w, h, bps), "%dx%d bd %d: tagged", w, h, bd);
  CHECK(tagged == (2 * w * h + pw * ph * bps <= kSrvTagBytes), "%dx%d bd %d: tagged rule", w, h, bd);
  const int need = srv_frac_need(tagged, w, h, bps);
  CHECK(need >= 1 && need < kSrvBlocks, "%dx%d bd %d: need %d", w, h, bd, need);
  // exactly blocks 1..need carry the sequence word (block 0's is the call's release, written last
  // by the caller), no block beyond
  CHECK(box->req[0][0] == 0, "%dx%d bd %d: req[0][0] written by the packer", w, h, bd);
  for (int p = 1; p < kSrvBlocks; p++)
    CHECK((box->req[p][0] == seq) == (p <= need), "%dx%d bd %d: block %d seq %u, need %d", w, h, bd, p, box->req[p][0], need);
  double got_ml;
  std::memcpy(&got_ml, &box->req[1][1], sizeof(got_ml));
  CHECK(got_ml == ml, "%dx%d bd %d: lambda", w, h, bd);
  CHECK((int16_t)(box->req[0][2] & 0xFFFFu) == -3 && (int16_t)(box->req[0][2] >> 16) == 5, "%dx%d bd %d: predictor", w, h, bd);

  // the kernel's LDS arrays, exactly sized: heap blocks, so a word past the end is an ASan error
  const int winw = srv_win_words(w, h, bps), totw = srv_payload_words(w, h, bps);
  std::vector<uint32_t> lwin((size_t)winw), lkey((size_t)(totw - winw));
  CHECK((size_t)(totw - winw) * 4 == (size_t)w * h * 2, "%dx%d bd %d: key words", w, h, bd);
  if (tagged) {
    for (int blk = 0; blk < kSrvBlocks; blk++)   // every polling lane, its two blocks
      srv_put_block(lwin.data(), lkey.data(), blk, need, winw, totw, box->req[blk][1], box->req[blk][2], box->req[blk][3]);
  } else {
    // 16-byte loads: each must lie inside SrvBox::win / SrvBox::key; the window's last may end in
    // win's padding, whole loads go to the LDS window (which has padding of its own)
    const int nwl = srv_win_loads(w, h, bps), nkl = srv_key_loads(w, h);
    CHECK((size_t)nwl * 16 <= sizeof(box->win), "%dx%d bd %d: window loads leave SrvBox::win", w, h, bd);
    CHECK((size_t)nwl * 16 >= (size_t)winw * 4 && (size_t)nwl * 16 < (size_t)winw * 4 + 16, "%dx%d bd %d: window loads", w, h, bd);
    CHECK((size_t)nkl * 16 == (size_t)w * h * 2 && (size_t)nkl * 16 <= sizeof(box->key), "%dx%d bd %d: key loads", w, h, bd);
    std::vector<uint32_t> tmp((size_t)nwl * 4);
    std::memcpy(tmp.data(), box->win, (size_t)nwl * 16);
    std::memcpy(lwin.data(), tmp.data(), (size_t)winw * 4);
    std::memcpy(lkey.data(), box->key, (size_t)nkl * 16);
  }
  // the largest window's last load against the structure (the bound the kernel relies on)
  CHECK((size_t)srv_win_loads(64, 64, bps) * 16 <= sizeof(box->win), "bd %d: 64x64 window loads", bd);

  // sample for sample against the clamped inputs
  const uint8_t* w8 = reinterpret_cast<const uint8_t*>(lwin.data());
  std::vector<uint16_t> w16((size_t)pw * ph);
  if (bps == 2) std::memcpy(w16.data(), lwin.data(), (size_t)pw * ph * 2);
  for (int y = 0; y < ph; y++)
    for (int x = 0; x < pw; x++) {
      int v = plane[(size_t)y * pw + x];
      v = v < 0 ? 0 : (v > maxv ? maxv : v);
      const int got = bps == 1 ? (int)w8[y * pw + x] : (int)w16[(size_t)y * pw + x];
      if (got != v) {
        CHECK(false, "%dx%d bd %d: window (%d, %d) %d != %d", w, h, bd, x, y, got, v);
        return;
      }
    }
  std::vector<int16_t> k16((size_t)w * h);
  std::memcpy(k16.data(), lkey.data(), (size_t)w * h * 2);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++)
      if (k16[(size_t)y * w + x] != key[(size_t)y * ks + x]) {
        CHECK(false, "%dx%d bd %d: key (%d, %d)", w, h, bd, x, y);
        return;
      }
}

int main() {
  static_assert(kSrvTagBytes == 1512, "tagged payload bound");
  static_assert(sizeof(SrvBox::win) >= 2 * 72 * 72 + 16, "window of 16-bit samples plus the tail padding");
  // the boundary the 10-bit payload crosses: 12x16 / 16x12 ride in the blocks, 16x16 does not
  static_assert(srv_fits_tagged(12, 16, 2) && srv_fits_tagged(16, 12, 2) && !srv_fits_tagged(16, 16, 2), "10-bit boundary");
  static_assert(srv_fits_tagged(16, 16, 1) && !srv_fits_tagged(32, 16, 1), "8-bit boundary");
  uint32_t seq = 7;
  int n = 0;
  for (const int bd : {8, 10})
    for (const auto& sh : kShapes) {
      one(sh[0], sh[1], bd, seq++);
      n++;
    }
  if (g_fail) {
    std::printf("srv pack: %d failures\n", g_fail);
    return 1;
  }
  std::printf("srv pack ok: %d shape x depth cases\n", n);
  return 0;
}
