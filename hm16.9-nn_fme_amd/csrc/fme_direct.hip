// fme_direct.hip — the two kernels of an NN-direct refinement batch (include/fme_direct.h) on gfx950,
// one source for 8 and 10 bits: the EMI square step on its own, and one sub-pel evaluation at the
// position NN_pred() names.  A batch is k_front (validation, tables, the tail's scan blocks), k_direct_emi,
// the ordinary NN tail (writer scan, net, status bits, state hand-over) and k_direct_eval, in stream
// order (direct_batch, fme_api.cpp).
//
// Lanes: k_cost_surface's (fme_surface.hip).  One lane per 4x4 unit; a job's lane group is its unit
// count rounded up to a power of two between 4 and 64 (a PU of more than 64 units walks them in
// steps of 64); a workgroup takes 64 consecutive jobs in call order, one per lane of its first wave,
// and packs their groups largest first.  Group sums go through the DPP / permlane steps; the
// group's first lane adds them to the job's row in LDS, and the lane of the first wave that holds
// the job finishes it and stores its record: no class grouping, no perm, no schedule.
//
// k_direct_emi: xTZ8PointSquareSearch at distance 1 around the TZ best as the lane kernels run it
// (fme_lane.hip section 1): the nine integer positions are priced from one 6x6 window per unit with
// the integer search's own metric (fme_tz_metric.h: SSE, or SAD12/24/48 with the FEN row
// subsampling; at 10 bits (d d) >> 4 per sample and the block's SAD >> 2), the eight neighbours are
// visited in the reference's order under its four range tests, each visited distortion is pushed,
// and the integer MV moves where distortion + MV cost (scale 2) is strictly less.  A job with
// FME_JOB_NN_IN takes its bound input row instead, a job with neither flag pushes nothing.
//
// k_direct_eval: the normative luma prediction of each unit at mv_int + the class's offset
// (fme_mc_luma.h luma_pred: fraction 0 in a direction is the filter-copy path, class 24 the integer
// position), FracDIF's distortion against the original or the key (fme_unit_target.h, fme_xlane.h
// unit_dist: SAD, 4x4 Hadamard, or the 8x8 Hadamard of a quad of lanes joined by two DPP butterfly
// stages), the PU's sum >> bitDepth - 8, the MV cost at scale 0 and xMotionEstimation's tail
// (me_tail, fme_device.h: the function tail_job calls).
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_direct_eval.h"
#include "fme_direct_host.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"
#include "fme_tz_metric.h"
#include "fme_unit_target.h"
#include "fme_xlane.h"

namespace fme {
namespace {

using namespace di;   // the lanes' per-job state and the evaluation (fme_direct_eval.h)

// ---- the EMI step's unit: the 6x6 window at rows and columns -1..4 and the nine positions ---------
// 8 bits: window rows of three dwords from the aligned column at or left of column -1 (s0: the byte
// shift of column -1), key rows as org bytes or int16 pairs.  part[p] = the unit's share of position
// p (0 centre, then TL, T, TR, L, R, BL, B, BR).
__device__ __forceinline__ int di_emi_dx(int p) { return (p == 1 || p == 4 || p == 6) ? -1 : ((p == 3 || p == 5 || p == 8) ? 1 : 0); }
__device__ __forceinline__ int di_emi_dy(int p) { return p >= 1 && p <= 3 ? -1 : (p >= 6 ? 1 : 0); }

template <bool k10>
__device__ __forceinline__ void di_emi_unit(const DiInfo& in, int x, int y, uint32_t (&part)[9]);

template <>
__device__ __forceinline__ void di_emi_unit<false>(const DiInfo& in, int x, int y, uint32_t (&part)[9]) {
  const bool kbuf = in.key != nullptr, sad = (in.mode & 1) != 0, sub = (in.mode & 2) != 0;
  uint32_t w[6][3];
  const uint32_t s0 = load_window<6, 3>(Plane{in.ref, in.rstride, in.pw, in.ph}, x + in.bx - 1, y + in.by - 1, in.ral != 0, w);
  uint32_t kk[4][2];
  int sk2 = 0;
  if (kbuf) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      g_sf_i16* kp = (g_sf_i16*)(in.key + (size_t)(y - in.y + r) * in.w + (x - in.x));
#pragma unroll
      for (int c = 0; c < 2; c++) kk[r][c] = (uint32_t)(uint16_t)kp[2 * c] | ((uint32_t)(uint16_t)kp[2 * c + 1] << 16);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint8_t* op = in.org + (size_t)(y + r) * in.ostride + x;
      uint32_t v;
      if (in.oal) {
        v = gld32(op);
      } else {
        v = gld8(op) | (gld8(op + 1) << 8) | (gld8(op + 2) << 16) | (gld8(op + 3) << 24);
      }
      kk[r][0] = v;
      kk[r][1] = 0u;
      sk2 = dot4(v ^ 0x80808080u, v ^ 0x80808080u, sk2);
    }
  }
#pragma unroll
  for (int p = 0; p < 9; p++) {
    // the position's rows 1 + dy .. 4 + dy of the window, from byte s0 + 1 + dx (0..5) of each
    const int dy = di_emi_dy(p);
    const uint32_t b = s0 + 1u + (uint32_t)di_emi_dx(p);
    const bool up1 = b >= 4u;   // (selects, not an indexed read: the window stays in registers)
    uint32_t q[4][2];
#pragma unroll
    for (int r = 0; r < 4; r++) {   // load_window gives (s - 128) bytes, the metric takes samples
      q[r][0] = (up1 ? w[r + 1 + dy][1] : w[r + 1 + dy][0]) ^ 0x80808080u;
      q[r][1] = (up1 ? w[r + 1 + dy][2] : w[r + 1 + dy][1]) ^ 0x80808080u;
    }
    part[p] = tzm::unit_part<4, 4, 2>(q, b & 3u, kk, sk2, kbuf, sad, sub);
  }
}

// 10 bits: window rows of four sample pairs from the even column at or left of column -1, the key
// rows as pairs (org samples or the int16 key).
template <>
__device__ __forceinline__ void di_emi_unit<true>(const DiInfo& in, int x, int y, uint32_t (&part)[9]) {
  const bool sad = (in.mode & 1) != 0, sub = (in.mode & 2) != 0;
  const uint16_t* pl = reinterpret_cast<const uint16_t*>(in.ref);
  const int x0 = x + in.bx - 1, y0 = y + in.by - 1, xa = x0 & ~1;
  const uint32_t s0 = (uint32_t)(x0 - xa);
  uint32_t w[6][4];
  const bool inside = xa >= 0 && xa + 8 <= in.pw && y0 >= 0 && y0 + 6 <= in.ph;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    const uint16_t* row = pl + (size_t)clamp_i(y0 + r, 0, in.ph - 1) * in.rstride;
    if (inside) {
      const di_u4 v = *(g_di_cu4*)(row + xa);
      w[r][0] = v.x; w[r][1] = v.y; w[r][2] = v.z; w[r][3] = v.w;
    } else {   // the padded picture: columns clamped
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t lo = *(const gu16c*)(row + clamp_i(xa + 2 * c, 0, in.pw - 1));
        const uint32_t hi = *(const gu16c*)(row + clamp_i(xa + 2 * c + 1, 0, in.pw - 1));
        w[r][c] = lo | (hi << 16);
      }
    }
  }
  uint32_t kk[4][2];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (in.key) {
      g_sf_i16* kp = (g_sf_i16*)(in.key + (size_t)(y - in.y + r) * in.w + (x - in.x));
#pragma unroll
      for (int c = 0; c < 2; c++) kk[r][c] = (uint32_t)(uint16_t)kp[2 * c] | ((uint32_t)(uint16_t)kp[2 * c + 1] << 16);
    } else {
      const gu16c* op = (const gu16c*)(reinterpret_cast<const uint16_t*>(in.org) + (size_t)(y + r) * in.ostride + x);
#pragma unroll
      for (int c = 0; c < 2; c++) kk[r][c] = (uint32_t)op[2 * c] | ((uint32_t)op[2 * c + 1] << 16);
    }
  }
#pragma unroll
  for (int p = 0; p < 9; p++) {
    const int dy = di_emi_dy(p);
    const uint32_t b = s0 + 1u + (uint32_t)di_emi_dx(p);   // sample 0..3 of the row
    const bool up1 = b >= 2u;
    uint32_t q[4][3];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) q[r][c] = up1 ? w[r + 1 + dy][c + 1] : w[r + 1 + dy][c];
    part[p] = tzm::unit_part10<4, 4>(q, b & 1u, kk, sad, sub);
  }
}

template <bool k10>
__global__ __launch_bounds__(kDiBlock) void k_direct_emi(DirectArgs d) {
  if (d.sched->invalid) return;   // a rejected batch: its jobs may name anything (workgroup-uniform)
  const BatchArgs& a = d.a;
  __shared__ DiInfo info[kDiTasks];
  __shared__ uint32_t e9s[kDiTasks][9];     // the jobs' nine distortions
  __shared__ uint8_t slot_task[kGroupSlots];   // job of each 4-lane slot
  __shared__ int total_lanes;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kDiTasks;
  const int nt = min(kDiTasks, d.n - t0);   // jobs of this workgroup (> 0 by the grid)
  for (int i = t; i < kDiTasks * 9; i += kDiBlock) (&e9s[0][0])[i] = 0u;
  fme_job j{};   // first wave: lane t keeps job t0 + t
  if (t < kDiTasks) {
    DiInfo& in = info[t];
    int lanes = 0;
    in.units = 0;
    in.uxn = 1;
    in.mode = 0;
    if (t < nt) {
      j = load_job(a, t0 + t);
      // FME_JOB_NN_IN takes precedence over FME_JOB_EMI, as in the lane kernels
      if ((j.flags & FME_JOB_EMI) && !(j.flags & FME_JOB_NN_IN)) {
        di_fill(a, j, in);
        const bool sad = j.w == 12 || j.w == 24 || j.w == 48;
        in.mode = (sad ? 1 : 0) | (sad && (a.fen == 1 || a.fen == 3) ? 2 : 0);   // (every such shape is taller than 8)
        in.bx = j.mv_x;
        in.by = j.mv_y;
        lanes = group_lanes(in.units);
      }
    }
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
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
    // a group of 64 lanes fills its wave, so the rounds of a wave's groups are 1 or all the same
    for (int u = li; __any(u < units); u += G) {   // wave-uniform
      const bool valid = u < units;
      uint32_t part[9];
#pragma unroll
      for (int p = 0; p < 9; p++) part[p] = 0u;
      if (valid) {
        const int uxn = max(in.uxn, 1);
        di_emi_unit<k10>(in, in.x + 4 * (u % uxn), in.y + 4 * (u / uxn), part);
      }
#pragma unroll
      for (int p = 0; p < 9; p++) {
        const uint32_t s = group_sum(part[p], G, lane);   // every lane of the wave is here
        if (valid && li == 0) e9s[q][p] += s;             // one writer per job: its group's first lane
      }
    }
  }
  __syncthreads();
  if (t >= nt) return;
  // ---- the decision (TEncSearch.cpp:1341-1376 visiting order and range checks, 1155-1188 update)
  // and the record's EMI fields, as the lane kernels leave them ----
  const int i = t0 + t;
  int mvx = j.mv_x, mvy = j.mv_y, n_emi = 0;
  uint32_t cval = 0, emi[8];
#pragma unroll
  for (int k = 0; k < 8; k++) emi[k] = 0u;
  if (j.flags & FME_JOB_NN_IN) {
    const g_di_u32* row = (const g_di_u32*)(a.nn_in + (size_t)9 * i);
#pragma unroll
    for (int k = 0; k < 8; k++) emi[k] = row[k];
    cval = row[8];
    n_emi = 8;
  } else if (j.flags & FME_JOB_EMI) {
    const DiInfo& in = info[t];
    const double ml = a.mlambda[j.lambda_id];
    // xGetSAD12/24/48 at bit depth 10: the block's sum >> 2
    const int sh = (k10 && (in.mode & 1)) ? d.bit_depth - 8 : 0;
    const int sx = mvx, sy = mvy;
    const uint32_t e0 = e9s[t][0] >> sh;
    uint32_t best = e0 + mv_cost(ml, mv_bits(sx, sy, 2, j.mvp_x, j.mvp_y));
    uint32_t best_cost = best - e0;
    const bool top = sy - 1 >= j.lt_y, bot = sy + 1 <= j.rb_y;
    const bool left = sx - 1 >= j.lt_x, right = sx + 1 <= j.rb_x;
#pragma unroll
    for (int p = 1; p <= 8; p++) {
      const int dx = di_emi_dx(p), dy = di_emi_dy(p);
      const bool ok = (dy == -1 ? top : (dy == 1 ? bot : true)) && (dx == -1 ? left : (dx == 1 ? right : true));
      if (ok) {
        const uint32_t dd = e9s[t][p] >> sh;
#pragma unroll
        for (int k = 0; k < 8; k++)   // emi[n_emi++] = dd with a static register index
          if (k == n_emi) emi[k] = dd;
        n_emi++;
        if (dd < best) {
          const uint32_t cst = mv_cost(ml, mv_bits(sx + dx, sy + dy, 2, j.mvp_x, j.mvp_y));
          const uint32_t dc = dd + cst;
          if (dc < best) {
            best = dc;
            best_cost = cst;
            mvx = sx + dx;
            mvy = sy + dy;
          }
        }
      }
    }
    cval = best - best_cost;
  }
  // the whole record: mv (tail), half / qtr, frac_cost, cost, bits (evaluation) are 0 until written;
  // frac_cost is a placeholder the tail prices and the evaluation replaces (direct_batch)
  g_di_u4* out = (g_di_u4*)(a.res + i);
  out[0] = di_u4{(uint32_t)(uint16_t)mvx | ((uint32_t)(uint16_t)mvy << 16), 0u, 0u, 0u};
  out[1] = di_u4{0u, 0u, cval, emi[0]};
  out[2] = di_u4{emi[1], emi[2], emi[3], emi[4]};
  out[3] = di_u4{emi[5], emi[6], emi[7], (uint32_t)n_emi};
}

}  // namespace

static_assert(sizeof(fme_result) == 64 && sizeof(fme_mv_result) == 16, "record layouts");

hipError_t launch_direct_emi(const DirectArgs& d, hipStream_t s) {
  return launch_by_depth(k_direct_emi<false>, k_direct_emi<true>, (d.n + kDiTasks - 1) / kDiTasks, kDiBlock, d, s);
}

hipError_t launch_direct_eval(const DirectArgs& d, hipStream_t s) {
  return launch_by_depth(k_direct_eval<false, DirectArgs>, k_direct_eval<true, DirectArgs>, (d.n + kDiTasks - 1) / kDiTasks, kDiBlock, d, s);
}

}  // namespace fme
