// fme_among.hip — the two kernels of candidate-set refinement (include/fme_among.h) on gfx950, one
// source for 8 and 10 bits.  fme_refine_among* is k_front, k_direct_emi (fme_direct.hip) unless the
// caller brings rows, then k_among_eval; fme_refine_topk* is k_front, k_direct_emi, k_nn_rows
// (fme_extern.hip), k_nn_rank, k_among_eval (among_batch, topk_batch, fme_api.cpp).
//
// k_among_eval: k_direct_eval's lanes (fme_direct_eval.h: one lane per 4x4 unit, a job's lane group
// its unit count rounded up to a power of two, 64 consecutive jobs per workgroup packed largest
// group first) with a loop over the job's k slots inside the unit.  The lane loads the 12x12
// reference window at rows and columns -4..+7 around the unit at the integer MV, and the target,
// once; every candidate of the job is predicted from that window.  The lanes of a wave belong to
// different jobs with different lists, and the group sums need every lane, so the slot loop is
// wave-uniform (s = 0 .. k - 1) and the position is a per-lane value.  The window is not shifted by
// the integer part of the offset (-1 or 0): the taps are.  An 8-tap filter at integer part ip reads
// window columns c + ip + 1 .. c + ip + 8, which is a 9-tap filter over columns c .. c + 8 whose
// first (ip = 0) or last (ip = -1) tap is 0: the same integer sum.  At 8 bits the first stage keeps
// its dot4 form, so there the window row is shifted by ip + 1 bytes (alignbyte with the shift in a
// VGPR) and the 8 taps stay; the second stage takes 9 taps at both depths.  A lane at an empty slot
// predicts class 24, contributes 0 and stores nothing.  Per-slot group sums go to the job's LDS row
// (8 words); behind the barrier one lane per job turns them into costs (the PU's sum >> bit depth
// - 8, + mv_cost), picks the first least, runs me_tail and writes the record in the three forms of
// k_direct_eval<., ExternArgs>, and the cand_cost words.
//
// k_nn_rank: one lane per row.  NN_pred()'s layers as nn_forward (fme_kernels.hip) has them, on the
// same packed weights through wave-uniform loads, restated here operation for operation (that file
// is not touched); the output loop keeps the 8 best (value, class) pairs sorted in registers by
// insertion with strict >, so equal values keep index order, and the first k go out.
#include <hip/hip_runtime.h>

#include "fme_among_host.h"
#include "fme_device.h"
#include "fme_direct_eval.h"

namespace fme {
namespace {

using namespace di;

// The unit's window and its prediction at a per-lane position: ix / iy = integer part + 1 (0 or 1),
// fx / fy the quarter-pel fractions.
template <bool k10>
struct AmWin;

template <>
struct AmWin<false> {
  uint32_t a[12][3];   // rows of (s - 128) bytes, re-aligned to the window's first column
  __device__ __forceinline__ void load(const DiInfo& in, int bx, int by, bool valid) {
    if (valid) {
      uint32_t w[12][4];
      const uint32_t s0 = load_window<12, 4>(Plane{in.ref, in.rstride, in.pw, in.ph}, bx - 4, by - 4, in.ral != 0, w);
#pragma unroll
      for (int r = 0; r < 12; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) a[r][k] = __builtin_amdgcn_alignbyte(w[r][k + 1], w[r][k], s0);
    } else {
#pragma unroll
      for (int r = 0; r < 12; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) a[r][k] = 0u;
    }
  }
  // stage 1 in the (s - 128) domain (UnitWin::pred): sum c.s - 8192, all 12 rows
  __device__ __forceinline__ void hstage(int ix, int fx, int (&t)[12][4]) const {
    uint32_t hlo, hhi;
    luma_taps(fx, hlo, hhi);
    const uint32_t sh = (uint32_t)ix;
#pragma unroll
    for (int r = 0; r < 12; r++) {
      // bytes ix .. ix + 11 of the row (the last one is read by no tap)
      const uint32_t s[3] = {__builtin_amdgcn_alignbyte(a[r][1], a[r][0], sh), __builtin_amdgcn_alignbyte(a[r][2], a[r][1], sh),
                             __builtin_amdgcn_alignbyte(0u, a[r][2], sh)};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int q = c + 4;
        const uint32_t b0 = (c & 3) ? __builtin_amdgcn_alignbyte(s[(c >> 2) + 1], s[c >> 2], (uint32_t)(c & 3)) : s[c >> 2];
        const uint32_t b1 = (q & 3) ? __builtin_amdgcn_alignbyte(s[(q >> 2) + 1], s[q >> 2], (uint32_t)(q & 3)) : s[q >> 2];
        t[r][c] = dot4(b1, hhi, dot4(b0, hlo, 0));
      }
    }
  }
  // stage 2, uni-pred (isLast): (sum + 2048 + (8192 << 6)) >> 12 clipped
  static __device__ __forceinline__ int finish(int sum) { return clamp_i((sum + 2048 + (8192 << 6)) >> 12, 0, 255); }
};

// The 8 taps of fraction f as 9 taps over a window that starts one sample early: i = 0 puts them at
// 0..7 (integer part -1), i = 1 at 1..8 (integer part 0).
__device__ __forceinline__ void taps9(int f, int i, int (&tp)[9]) {
  uint32_t lo, hi;
  luma_taps(f, lo, hi);
  int t8[8];
#pragma unroll
  for (int k = 0; k < 8; k++) t8[k] = tap_of(lo, hi, k);
#pragma unroll
  for (int k = 0; k < 9; k++) tp[k] = i ? (k >= 1 ? t8[k - 1] : 0) : (k < 8 ? t8[k] : 0);
}

template <>
struct AmWin<true> {
  int sv[12][12];   // s - 512
  __device__ __forceinline__ void load(const DiInfo& in, int bx, int by, bool valid) {
    const uint16_t* pl = reinterpret_cast<const uint16_t*>(in.ref);
#pragma unroll
    for (int r = 0; r < 12; r++)
#pragma unroll
      for (int c = 0; c < 12; c++) sv[r][c] = 0;
    if (!valid) return;
#pragma unroll
    for (int r = 0; r < 12; r++) {
      const gu16c* row = (const gu16c*)(pl + (size_t)clamp_i(by - 4 + r, 0, in.ph - 1) * in.rstride);
#pragma unroll
      for (int c = 0; c < 12; c++) sv[r][c] = (int)row[clamp_i(bx - 4 + c, 0, in.pw - 1)] - 512;
    }
  }
  // stage 1 at bit depth 10 (pred10): (sum c.s') >> 2, all 12 rows
  __device__ __forceinline__ void hstage(int ix, int fx, int (&t)[12][4]) const {
    int tp[9];
    taps9(fx, ix, tp);
#pragma unroll
    for (int r = 0; r < 12; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) acc += tp[k] * sv[r][c + k];
        t[r][c] = acc >> 2;
      }
  }
  // stage 2, uni-pred (isLast): ((sum + 512) >> 10) + 512 clipped
  static __device__ __forceinline__ int finish(int sum) { return clamp_i(((sum + 512) >> 10) + 512, 0, 1023); }
};

// Slot s of a job's list (two words, slot 0 in the low byte of the first).
__device__ __forceinline__ int list_slot(uint32_t lo, uint32_t hi, int s) {
  return (int)(((s < 4 ? lo : hi) >> (8 * (s & 3))) & 0xFFu);
}

template <bool k10>
__global__ __launch_bounds__(kDiBlock) void k_among_eval(AmongArgs x) {
  const DirectArgs& d = x.d;
  const BatchArgs& a = d.a;
  const int K = x.k;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kDiTasks;
  const int nt = min(kDiTasks, d.n - t0);   // jobs of this workgroup (> 0 by the grid)
  if (d.sched->invalid) {   // a rejected batch: every record marked, 0 otherwise; the costs all ones
    if (t < nt) {
      const di_u4 z{0u, 0u, 0u, 0u}, st{0u, 0u, 0u, (uint32_t)FME_RES_REJECTED << 16};
      if (d.mv_out) {
        *(g_di_u4*)(d.mv_out + t0 + t) = st;
      } else {
        g_di_u4* r = (g_di_u4*)(a.res + t0 + t);
        r[0] = z; r[1] = z; r[2] = z; r[3] = st;
      }
      if (x.cand_cost)
        for (int s = 0; s < K; s++) ((g_di_u32*)x.cand_cost)[(size_t)(t0 + t) * K + s] = kAmongNone;
    }
    return;
  }
  __shared__ DiInfo info[kDiTasks];
  __shared__ uint32_t lists[kDiTasks][2];
  __shared__ uint32_t dist[kDiTasks][FME_AMONG_MAX];
  __shared__ uint8_t slot_task[kGroupSlots];
  __shared__ int total_lanes;
  fme_job j{};   // first wave: lane t keeps job t0 + t, its integer MV, list and the record's EMI fields
  int mvx = 0, mvy = 0;
  uint32_t llo = 0xFFFFFFFFu, lhi = 0xFFFFFFFFu;   // the list, unused slots empty
  uint32_t last = 0, row_status = 0;
  bool refused = false;
  fme_result from_row{};
  if (t < kDiTasks) {
    DiInfo& in = info[t];
    int lanes = 0;
#pragma unroll
    for (int s = 0; s < FME_AMONG_MAX; s++) dist[t][s] = 0u;
    in.units = 0;
    in.uxn = 1;
    in.mode = kDistSad;
    if (t < nt) {
      j = load_job(a, t0 + t);
      const uint8_t* cl = x.cand + (size_t)(t0 + t) * K;
      bool any = false;
#pragma unroll
      for (int s = 0; s < FME_AMONG_MAX; s++) {
        if (s < K) {
          const uint32_t v = gld8(cl + s);
          refused = refused || !among_slot_ok((int)v);
          any = any || !among_slot_empty((int)v);
          if (s < 4) llo = (llo & ~(0xFFu << (8 * s))) | (v << (8 * s));
          else lhi = (lhi & ~(0xFFu << (8 * (s - 4)))) | (v << (8 * (s - 4)));
        }
      }
      refused = refused || !any;
      if (x.rows) {
        const di_u4 q0 = di_ld16(x.rows + t0 + t, 0), q1 = di_ld16(x.rows + t0 + t, 1);
        const di_u4 q2 = di_ld16(x.rows + t0 + t, 2), q3 = di_ld16(x.rows + t0 + t, 3);
        const uint32_t qw[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                 q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
        fme_nn_row row;
        __builtin_memcpy(&row, qw, sizeof(row));
        refused = refused || !extern_row_ok(row, j.mv_x, j.mv_y);
        extern_row_record(row, from_row);
        mvx = from_row.mv_int_x;
        mvy = from_row.mv_int_y;
        last = from_row.n_emi;
        row_status = row.status & (uint32_t)(FME_RES_NN_STALE | FME_RES_NN_UNINIT);
      } else {
        const g_di_u32* rec = (const g_di_u32*)(a.res + t0 + t);
        const uint32_t mvw = rec[0];
        last = rec[15] & 0xFFu;   // n_emi
        mvx = (int16_t)(mvw & 0xFFFFu);
        mvy = (int16_t)(mvw >> 16);
      }
      if (!refused) {
        di_fill(a, j, in);
        in.bx = mvx;
        in.by = mvy;
        in.fx = 0;
        in.fy = 0;
        in.mode = dist_mode(a.use_hadamard && !(j.flags & FME_JOB_LOSSLESS), j.w, j.h);
        lanes = group_lanes(in.units);
      }
    }
    lists[t][0] = llo;
    lists[t][1] = lhi;
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
    const unsigned long long m = __ballot(refused);   // the first wave, all of it: one count per workgroup
    if (lane == 0 && m) atomicAdd(x.refused, (int)__popcll(m));
  }
  __syncthreads();
  const int total = total_lanes;
  for (int g0 = 0; g0 < total; g0 += kDiBlock) {   // workgroup-uniform
    const int g = g0 + t;
    const bool act = g < total;
    const int q = act ? (int)slot_task[g >> 2] : 0;
    const DiInfo& in = info[q];
    const int G = act ? in.lanes : 64;
    const int li = g - in.start;
    const int units = act ? in.units : 0;
    const uint32_t qlo = lists[q][0], qhi = lists[q][1];
    for (int u = li; __any(u < units); u += G) {   // wave-uniform
      const bool valid = u < units;
      const int mode = in.mode, uxn = max(in.uxn, 1);
      int ux, uy;
      unit_xy(u, uxn, mode == kDistHad8, ux, uy);
      const int px = in.x + 4 * ux, py = in.y + 4 * uy;
      AmWin<k10> win;
      win.load(in, px + in.bx, py + in.by, valid);
      int o[4][4];
      unit_target<k10>(in, px, py, valid, o);
      for (int s = 0; s < K; s++) {   // uniform: the position is the lane's
        const int v = list_slot(qlo, qhi, s);
        const bool on = valid && !among_slot_empty(v);
        const int cls = on ? v : 24;
        const int ox = direct_dx(cls), oy = direct_dy(cls);
        int tt[12][4];
        win.hstage(direct_int(ox) + 1, direct_frac(ox), tt);
        int vp[9];
        taps9(direct_frac(oy), direct_int(oy) + 1, vp);
        int df[4][4];
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
          for (int c = 0; c < 4; c++) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) sum += tt[y + k][c] * vp[k];
            df[y][c] = o[y][c] - AmWin<k10>::finish(sum);
          }
        // the lanes of a quad share a job and a round: the cross-lane stages of an 8x8 tile see all four
        uint32_t acc = unit_dist(df, mode, lane, (u & 3) == 0);
        if (!on) acc = 0;
        acc = group_sum(acc, G, lane);   // wave-uniform control flow: every lane of the wave is here
        if (on && li == 0) dist[q][s] += acc;   // one writer per job: its group's first lane
      }
    }
  }
  __syncthreads();
  if (t >= nt) return;
  // ---- the slots' costs, the pick, the tail, the record ----
  const int i = t0 + t;
  g_di_u32* cc = x.cand_cost ? (g_di_u32*)x.cand_cost + (size_t)i * K : nullptr;
  if (refused) {   // this job alone: 0 but for the status
    const di_u4 z{0u, 0u, 0u, 0u}, st{0u, 0u, 0u, (uint32_t)FME_RES_REJECTED << 16};
    if (d.mv_out) {
      *(g_di_u4*)(d.mv_out + i) = st;
    } else {
      g_di_u4* r = (g_di_u4*)(a.res + i);
      r[0] = z; r[1] = z; r[2] = z; r[3] = st;
    }
    if (cc)
      for (int s = 0; s < K; s++) cc[s] = kAmongNone;
    return;
  }
  const double ml = a.mlambda[j.lambda_id];
  const int sh = k10 ? d.bit_depth - 8 : 0;
  int cls = 24;
  uint32_t frac_cost = 0;
  bool have = false;
  for (int s = 0; s < K; s++) {
    const int v = list_slot(llo, lhi, s);
    uint32_t cs = kAmongNone;
    if (!among_slot_empty(v)) {
      cs = (dist[t][s] >> sh) + mv_cost(ml, mv_bits(4 * mvx + direct_dx(v), 4 * mvy + direct_dy(v), 0, j.mvp_x, j.mvp_y));
      if (!have || cs < frac_cost) {   // the first least, in slot order
        have = true;
        frac_cost = cs;
        cls = v;
      }
    }
    if (cc) cc[s] = cs;
  }
  const int fx = 4 * mvx + direct_dx(cls), fy = 4 * mvy + direct_dy(cls);
  uint32_t bits;
  const uint32_t cost = me_tail(j, ml, frac_cost, fx, fy, bits);
  const uint32_t status = x.status | (x.row_status ? row_status : 0u);
  const uint32_t mvw = (uint32_t)(uint16_t)fx | ((uint32_t)(uint16_t)fy << 16);
  if (d.mv_out) {
    *(g_di_u4*)(d.mv_out + i) = di_u4{mvw, cost, bits, (uint32_t)cls | (status << 16)};
  } else {
    uint8_t* r = reinterpret_cast<uint8_t*>(a.res + i);
    const di_u4 r0{(uint32_t)(uint16_t)mvx | ((uint32_t)(uint16_t)mvy << 16), mvw, direct_half_qtr_word(cls), frac_cost};
    const uint32_t w15 = (last & 0xFFu) | ((uint32_t)cls << 8) | (status << 16);
    if (x.rows) {   // the whole record: the EMI fields are the row's
      g_di_u4* o = (g_di_u4*)r;
      o[0] = r0;
      o[1] = di_u4{cost, bits, from_row.c, from_row.emi[0]};
      o[2] = di_u4{from_row.emi[1], from_row.emi[2], from_row.emi[3], from_row.emi[4]};
      o[3] = di_u4{from_row.emi[5], from_row.emi[6], from_row.emi[7], w15};
    } else {
      *(g_di_u4*)r = r0;
      *(g_di_u2*)(r + 16) = di_u2{cost, bits};
      *(g_di_u32*)(r + 60) = w15;
    }
  }
}

// ---- the ranking -----------------------------------------------------------------------------------
constexpr int kRankNT = 64;

// The 8 best (value, class) pairs, best first, in registers: among_insert (fme_among_host.h) with
// every index static.
struct Best8 {
  float val[FME_AMONG_MAX];
  uint32_t cls[FME_AMONG_MAX];
  int filled;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int q = 0; q < FME_AMONG_MAX; q++) {
      val[q] = 0.0f;
      cls[q] = FME_AMONG_EMPTY;
    }
    filled = 0;
  }
  __device__ __forceinline__ void insert(float v, uint32_t c) {
    int p = filled;   // in front of the held values it beats (strict >), from the back
#pragma unroll
    for (int q = FME_AMONG_MAX - 1; q >= 0; q--)
      if (q < filled && p == q + 1 && v > val[q]) p = q;
#pragma unroll
    for (int q = FME_AMONG_MAX - 1; q >= 1; q--)
      if (q > p) {
        val[q] = val[q - 1];
        cls[q] = cls[q - 1];
      }
#pragma unroll
    for (int q = 0; q < FME_AMONG_MAX; q++)
      if (q == p) {
        val[q] = v;
        cls[q] = c;
      }
    filled = min(filled + 1, FME_AMONG_MAX);
  }
};

__global__ __launch_bounds__(kRankNT) void k_nn_rank(const fme_nn_row* rows, const float* __restrict__ Q, uint8_t* cand,
                                                     int k, int n) {
  const int i = (int)blockIdx.x * kRankNT + (int)threadIdx.x;
  if (i >= n) return;
  const di_u4 q0 = di_ld16(rows + i, 0), q1 = di_ld16(rows + i, 1), q2 = di_ld16(rows + i, 2), q3 = di_ld16(rows + i, 3);
  Best8 b;
  b.init();
  if (!((q3.x >> 16) & FME_RES_REJECTED)) {
    // NN_pred() as nn_forward has it: float32, every dot product in k order, no contraction
    const int t = emb_row_h((int)q2.y) * 8 + emb_row_w((int)q2.z);
    float in[9];
    const uint32_t raw[9] = {q0.x, q0.y, q0.z, q0.w, q2.x, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int kk = 0; kk < 9; kk++) {
      float v = (float)raw[kk];
      v = (v - Q[kNnPkMean + kk]) / Q[kNnPkStd + kk];
      in[kk] = v * Q[kNnPkGin + kk];
    }
    const float* pfx = Q + kNnPkPfx + t * 22;
    f2 x1[11];
#pragma unroll
    for (int rp = 0; rp < 11; rp++) {
      f2 s = {pfx[2 * rp], pfx[2 * rp + 1]};
#pragma unroll
      for (int kk = 0; kk < 9; kk++) s = s + ld2(Q, kNnPkW1 + (rp * 9 + kk) * 2) * (f2){in[kk], in[kk]};
      s = relu2(s + ld2(Q, kNnPkB1 + 2 * rp));
      x1[rp] = s * ld2(Q, kNnPkG1 + 2 * rp) + ld2(Q, kNnPkBE1 + 2 * rp);
    }
    f2 x2[10];
#pragma unroll
    for (int rp = 0; rp < 10; rp++) {
      f2 s = {0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < 22; kk++) {
        const float xk = (kk & 1) ? x1[kk / 2].y : x1[kk / 2].x;
        s = s + ld2(Q, kNnPkW2 + (rp * 22 + kk) * 2) * (f2){xk, xk};
      }
      s = relu2(s + ld2(Q, kNnPkB2 + 2 * rp));
      x2[rp] = s * ld2(Q, kNnPkG2 + 2 * rp) + ld2(Q, kNnPkBE2 + 2 * rp);
    }
#pragma unroll 1   // the weights of one row pair per iteration (scalar loads, few SGPRs)
    for (int rp = 0; rp < 25; rp++) {
      f2 s = {0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < 20; kk++) {
        const float xk = (kk & 1) ? x2[kk / 2].y : x2[kk / 2].x;
        s = s + ld2(Q, kNnPkW3 + (rp * 20 + kk) * 2) * (f2){xk, xk};
      }
      s = s + ld2(Q, kNnPkBout + 2 * rp);
      b.insert(s.x, (uint32_t)(2 * rp));
      if (rp < 24) b.insert(s.y, (uint32_t)(2 * rp + 1));
    }
  }
  uint8_t* out = cand + (size_t)i * k;
  const uint32_t lo = b.cls[0] | (b.cls[1] << 8) | (b.cls[2] << 16) | (b.cls[3] << 24);
  const uint32_t hi = b.cls[4] | (b.cls[5] << 8) | (b.cls[6] << 16) | (b.cls[7] << 24);
  if (k == FME_AMONG_MAX && ((uintptr_t)cand & 7u) == 0) {   // the job's whole list: one 8-byte store
    *(g_di_u2*)out = di_u2{lo, hi};
  } else {   // k bytes, none beyond
    typedef __attribute__((address_space(1))) uint8_t g_u8;
    for (int s = 0; s < k; s++) ((g_u8*)out)[s] = (uint8_t)list_slot(lo, hi, s);
  }
}

}  // namespace

hipError_t launch_among_eval(const AmongArgs& x, hipStream_t s) {
  return launch_by_depth(k_among_eval<false>, k_among_eval<true>, (x.n + kDiTasks - 1) / kDiTasks, kDiBlock, x, s);
}

hipError_t launch_nn_rank(const fme_nn_row* rows, const float* nn_params, uint8_t* cand, int k, int n, hipStream_t s) {
  if (n > 0)
    hipLaunchKernelGGL(k_nn_rank, dim3((n + kRankNT - 1) / kRankNT), dim3(kRankNT), 0, s, rows, nn_params, cand, k, n);
  return hipGetLastError();
}

}  // namespace fme
