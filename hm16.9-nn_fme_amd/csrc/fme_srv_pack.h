// fme_srv_pack.h — the single-call server's mailbox: its layout, how many request blocks a call
// uses and where each payload word of a block goes, in ONE place for the host that packs a request
// (fme_api.cpp) and the resident kernel that waits for it and unpacks it (fme_server.hip).  The
// kernel waits until every block the call uses carries the call's sequence word; a host that packed
// fewer blocks than the kernel counts would leave the workgroup waiting until the host's bound
// expires, so both sides call the same functions and tests/cpp/test_srv_pack.cpp runs the pair
// against each other on a CPU for every PU shape and both bit depths.
//
// Depends on <cstdint> / <cstring> only; FME_SRV_HD is empty without hipcc.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FME_SRV_HD __host__ __device__
#else
#define FME_SRV_HD
#endif

namespace fme {

// One resident workgroup polls the request blocks of this structure in pinned, device-mapped host
// memory, serves the call and stores the answer block `res`; `stopped` = the epoch of an instance
// that exited (idle, lifetime or `stop`).  Request fields share the first lines, the answer has its
// own, the payload follows.
enum { kSrvNn = 1, kSrvFrac = 2, kSrvSad = 4, kSrvTagged = 8, kSrvMarks = 16 };
constexpr int kSrvBlocks = 128;                       // request blocks, all read by every poll
constexpr int kSrvTagBytes = 12 * (kSrvBlocks - 2);   // FracDIF payload that rides in the blocks
constexpr int kSrvMaxPu = 64;                         // largest PU side
constexpr int kSrvMaxWin = (kSrvMaxPu + 8) * (kSrvMaxPu + 8);   // samples of the largest window
struct SrvBox {
  // host -> device, in 16-byte blocks that the polling wave reads all at once (two per lane, one
  // load each), so a block's fields are those written before its sequence word.  req[0]: seq,
  // shape = kind (bits 0-1) | kSrvSad (lossless or HADME off) | kSrvTagged | kSrvMarks (record the
  // phase checkpoints in `marks`) | w - 1 (bits 8-15) |
  // h - 1 (bits 16-23), the FracDIF predictor - 4 * integer MV (x low 16 bits, y high 16,
  // quarter-pel), stop (set by the host to end the instance).  The rest carry this call's seq in
  // word 0 and are taken only when every one the call uses does:
  //   NN_pred: req[1..4], three inputs each (array_e[8], C, PUHeight, PUWidth);
  //   FracDIF: req[1] = the motion lambda (TComRdCost::m_motionLambda, a double in words 1-2);
  //   kSrvTagged: req[2..] = the window then the key, 12 bytes per block, when they fit in
  //   kSrvTagBytes (the payload arrives with the request: no second round trip); otherwise they are
  //   in key / win below, read after the request.
  // The bit depth is the context's (one server instance serves one depth), not a request field:
  // window samples are uint8_t at bit depth 8 and uint16_t above.
  alignas(64) uint32_t req[kSrvBlocks][4];
  // device -> host, one 16-byte store: seq, FracDIF cost / NN class, FracDIF half x, y and quarter
  // x, y as int8 (bytes 0..3), the call's device ticks (request read to answer)
  alignas(64) uint32_t res[4];
  uint32_t marks[4];           // FracDIF checkpoints of the call (fme_single_last_device_us)
  uint32_t stopped;
  alignas(64) int16_t key[kSrvMaxPu * kSrvMaxPu];   // w * h (a multiple of 16 bytes for every PU shape)
  // (w + 8) x (h + 8) window around the integer MV, stride w + 8, in samples of the context's depth;
  // 16 bytes of padding: the kernel's last 16-byte load of a window may end inside it
  alignas(16) uint8_t win[2 * kSrvMaxWin + 16];
};

FME_SRV_HD constexpr int srv_bps(int bit_depth) { return bit_depth > 8 ? 2 : 1; }   // bytes per window sample
FME_SRV_HD constexpr int srv_win_bytes(int w, int h, int bps) { return (w + 8) * (h + 8) * bps; }
FME_SRV_HD constexpr int srv_key_bytes(int w, int h) { return 2 * w * h; }
// 32-bit words of the window, and of window + key (both whole: w and h are multiples of 4)
FME_SRV_HD constexpr int srv_win_words(int w, int h, int bps) { return srv_win_bytes(w, h, bps) >> 2; }
FME_SRV_HD constexpr int srv_payload_words(int w, int h, int bps) { return srv_win_words(w, h, bps) + (srv_key_bytes(w, h) >> 2); }
// does the payload ride in the request blocks?
FME_SRV_HD constexpr bool srv_fits_tagged(int w, int h, int bps) {
  return srv_win_bytes(w, h, bps) + srv_key_bytes(w, h) <= kSrvTagBytes;
}
// The last request block of a FracDIF call: blocks 1..need must all carry the call's sequence word
// (block 1 the motion lambda; tagged: blocks 2..need the payload, 12 bytes each).
FME_SRV_HD constexpr int srv_frac_need(bool tagged, int w, int h, int bps) {
  return tagged ? 1 + (srv_win_bytes(w, h, bps) + srv_key_bytes(w, h) + 11) / 12 : 1;
}
// Untagged: 16-byte loads that fetch the window (the last may end in SrvBox::win's padding) and the key.
FME_SRV_HD constexpr int srv_win_loads(int w, int h, int bps) { return (srv_win_bytes(w, h, bps) + 15) >> 4; }
FME_SRV_HD constexpr int srv_key_loads(int w, int h) { return srv_key_bytes(w, h) >> 4; }

// Payload words 1..3 (x) of request block blk: word k is payload word 3 * (blk - 2) + k, the window's
// words first, then the key's; blocks outside 2..need and words past the payload's end are dropped.
FME_SRV_HD inline void srv_put_block(uint32_t* win_words, uint32_t* key_words, int blk, int need, int winw, int totw,
                                     uint32_t x0, uint32_t x1, uint32_t x2) {
  if (blk < 2 || blk > need) return;
  const uint32_t x[3] = {x0, x1, x2};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 3; k++) {
    const int q = 3 * (blk - 2) + k;
    if (q < winw) win_words[q] = x[k];
    else if (q < totw) key_words[q - winw] = x[k];
  }
}

// Host: everything of a FracDIF request but req[0][0] (the call's release, srv_call): the window
// (rows -4..h+3, columns -4..w+3 around mv_int of the padded plane `ref`, clamped to the depth's
// sample range) and the key, in the request blocks when they fit, else in win / key; the lambda
// block; the shape and predictor words.  px, py: the MV predictor less 4 * mv_int (quarter-pel).
inline void srv_pack_frac(SrvBox* b, uint32_t seq, int bit_depth, bool lossless_or_sad, bool marks, const int16_t* key,
                          int key_stride, int w, int h, const int16_t* ref, int ref_stride, int mv_int_x, int mv_int_y,
                          int px, int py, double motion_lambda) {
  const int bps = srv_bps(bit_depth), pw = w + 8, ph = h + 8;
  const int win_bytes = srv_win_bytes(w, h, bps), bytes = win_bytes + srv_key_bytes(w, h);
  const bool tagged = srv_fits_tagged(w, h, bps);
  alignas(16) uint8_t stream[kSrvTagBytes + 12];
  if (tagged) std::memset(stream + bytes, 0, 12);   // the last block's words past the payload
  uint8_t* wdst = tagged ? stream : b->win;
  int16_t* kdst = tagged ? reinterpret_cast<int16_t*>(stream + win_bytes) : b->key;
  for (int y = 0; y < h; y++) std::memcpy(kdst + y * w, key + (intptr_t)y * key_stride, (size_t)w * sizeof(int16_t));
  const int maxv = (1 << bit_depth) - 1;
  for (int y = 0; y < ph; y++) {
    const int16_t* src = ref + (intptr_t)(mv_int_y - 4 + y) * ref_stride + (mv_int_x - 4);
    if (bps == 1) {
      uint8_t* dst = wdst + y * pw;
      for (int x = 0; x < pw; x++) dst[x] = (uint8_t)(src[x] < 0 ? 0 : (src[x] > 255 ? 255 : src[x]));
    } else {
      uint16_t* dst = reinterpret_cast<uint16_t*>(wdst) + y * pw;
      for (int x = 0; x < pw; x++) dst[x] = (uint16_t)(src[x] < 0 ? 0 : (src[x] > maxv ? maxv : src[x]));
    }
  }
  if (tagged)
    for (int p = 0; 12 * p < bytes; p++) {
      std::memcpy(&b->req[2 + p][1], stream + 12 * p, 12);
      __atomic_store_n(&b->req[2 + p][0], seq, __ATOMIC_RELEASE);
    }
  uint32_t mlw[2];
  std::memcpy(mlw, &motion_lambda, sizeof(mlw));
  b->req[1][1] = mlw[0];
  b->req[1][2] = mlw[1];
  __atomic_store_n(&b->req[1][0], seq, __ATOMIC_RELEASE);
  b->req[0][1] = (uint32_t)kSrvFrac | (lossless_or_sad ? (uint32_t)kSrvSad : 0u) | (tagged ? (uint32_t)kSrvTagged : 0u) |
                 (marks ? (uint32_t)kSrvMarks : 0u) | ((uint32_t)(w - 1) << 8) | ((uint32_t)(h - 1) << 16);
  b->req[0][2] = (uint32_t)(uint16_t)px | ((uint32_t)(uint16_t)py << 16);
}

}  // namespace fme
