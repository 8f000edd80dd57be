// fme_merge.hip — xGetInterPredictionError on the GPU (gfx950): the luma prediction of a PU's motion
// and its distortion against the original, fused, with no prediction plane written.
//
// One task = TEncSearch::xGetInterPredictionError (TEncSearch.cpp:3576-3596) for one PU and one
// motion (a merge candidate or the ME result):
//   * prediction: k_mc's luma path (fme_mc_luma.h): clipMv per list, xCheckIdenticalMotion,
//     xPredInterBlk uni (clipped to the bit depth) or bi (14-bit values, TComYuv::addAvg);
//   * distortion: setDistParam(DistParam&, bitDepth, org, pred, w, h, bHadamard)
//     (TComRdCost.cpp:277-290: iStep 1, iSubShift 0).  bHadamard (HADME on, CU not lossless):
//     xGetHADs (1428-1494): 8x8 Hadamards ((sum |coef| + 2) >> 2 each, xCalcHADs8x8 1330-1425) when
//     w and h are multiples of 8, else 4x4 ((sum |coef| + 1) >> 1 each, xCalcHADs4x4 1234-1328);
//     otherwise the SAD over every row (xGetSAD / xGetSAD4..64: the same full sum at every width).
//     The PU's sum is shifted right by bitDepth - 8 once (DISTORTION_PRECISION_ADJUSTMENT).
//
// Lanes: one per 4x4 unit.  A task's lane group is its unit count rounded up to a power of two,
// between 4 and 64 lanes (a PU of more than 64 units walks them in steps of 64); a workgroup takes
// 64 consecutive tasks and packs their groups into its lanes largest class first, so every group
// starts at a multiple of its size, never straddles a wave, and an 8x4 PU takes 4 lanes, not a
// wave.  With 8x8 Hadamards the units are ordered so that the four quadrants of an 8x8 block sit in
// four consecutive lanes: each lane transforms its 4x4 quadrant in registers, and two cross-lane
// butterfly stages over the quad (lane ^ 1, lane ^ 2; DPP quad_perm) turn the quadrants'
// transforms TA, TB, TC, TD into the 8x8 coefficients TA +- TB +- TC +- TD (the sum of absolute
// values does not depend on HM's butterfly order).  Integer arithmetic throughout: a 10-bit 8x8
// coefficient reaches 64 * 1023.
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"
#include "fme_xlane.h"

namespace fme {
namespace {

using namespace simd;
using namespace mcl;
using namespace xlane;

constexpr int kPeBlock = 256;
constexpr int kPeTasks = kGroupTasks;   // consecutive tasks per workgroup, set up by its first wave

// Per-task state shared by the workgroup (LDS), filled by one thread per task.
struct PeInfo {
  const uint8_t* ref[2];
  const uint8_t* org;
  int rstride[2], ral[2];     // reference stride, dword-aligned rows
  int ostride, oal;
  int pw, ph;                 // picture size (the original's and the references')
  int x, y, uxn, units;
  int lanes, start;           // lane group size (0: no work) and first lane slot
  int nl, mode;
  int ix[2], iy[2], fx[2], fy[2];
};

__device__ __forceinline__ bool pe_task_valid(const PeArgs& a, const fme_pe_task& t) {
  if (!pu_shape_ok(t.w, t.h)) return false;
  if (!(t.flags & (FME_MC_L0 | FME_MC_L1)) || (t.flags & ~(FME_MC_L0 | FME_MC_L1 | FME_PE_LOSSLESS))) return false;
  if (t.org_id >= FME_MAX_PICTURES) return false;
  const PicDesc& o = a.pics[t.org_id];
  if (!o.luma || (int)t.x + t.w > o.width || (int)t.y + t.h > o.height) return false;
  return refs_ok(t.flags, t.ref_id, a.pics, o.width, o.height, false);
}

// The prediction of the 4x4 unit at (x, y): both lists in registers, averaged (k_mc's luma block).
template <bool k10>
__device__ __forceinline__ void pe_predict(const PeInfo& in, int x, int y, int (&p)[4][4]) {
  const bool uni = in.nl == 1;
  pred_lists<k10>(in.nl, [&](int k, int (&o)[4][4]) {
    luma_pred<k10>(Plane{in.ref[k], in.rstride[k], in.pw, in.ph}, in.ral[k] != 0, x + in.ix[k], y + in.iy[k], in.fx[k],
                   in.fy[k], uni, o);
  }, p);
}

// d = org - pred of the unit at (x, y) (inside the original: the task was validated)
template <bool k10>
__device__ __forceinline__ void pe_diff(const PeInfo& in, int x, int y, const int (&p)[4][4], int (&d)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if constexpr (k10) {
      const gu16c* op = (const gu16c*)(reinterpret_cast<const uint16_t*>(in.org) + (size_t)(y + r) * in.ostride + x);
#pragma unroll
      for (int c = 0; c < 4; c++) d[r][c] = (int)op[c] - p[r][c];
    } else {
      const uint8_t* op = in.org + (size_t)(y + r) * in.ostride + x;
      if (in.oal) {   // x is a multiple of 4
        const uint32_t v = gld32(op);
#pragma unroll
        for (int c = 0; c < 4; c++) d[r][c] = (int)((v >> (8 * c)) & 255u) - p[r][c];
      } else {
#pragma unroll
        for (int c = 0; c < 4; c++) d[r][c] = (int)gld8(op + c) - p[r][c];
      }
    }
  }
}

template <bool k10>
__global__ __launch_bounds__(kPeBlock) void k_pred_err(PeArgs a) {
  __shared__ PeInfo info[kPeTasks];
  __shared__ uint8_t slot_task[kGroupSlots];   // task of each 4-lane slot
  __shared__ int total_lanes;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kPeTasks;
  if (t < kPeTasks) {   // the first wave: one task per lane
    PeInfo& in = info[t];
    int lanes = 0;
    const int ti = t0 + t;
    if (ti < a.n) {
      const fme_pe_task j = a.tasks[ti];
      if (!pe_task_valid(a, j)) {
        atomicAdd(a.invalid, 1);
        a.dist[ti] = 0xFFFFFFFFu;
      } else {
        ListMotion lm[2];
        const int nl = resolve_lists(j.flags, j.ref_id, j.mv, j.cu_x, j.cu_y, a.pics, true, lm);
        in.nl = nl;
        const PicDesc o = a.pics[j.org_id];
#pragma unroll
        for (int k = 0; k < 2; k++) {
          if (k >= nl) break;
          in.ix[k] = lm[k].lix;
          in.iy[k] = lm[k].liy;
          in.fx[k] = lm[k].lfx;
          in.fy[k] = lm[k].lfy;
          in.ref[k] = lm[k].pic.luma;
          in.rstride[k] = lm[k].pic.stride;
          in.ral[k] = dword_rows(lm[k].pic.luma, lm[k].pic.stride);
        }
        in.org = o.luma;
        in.ostride = o.stride;
        in.oal = dword_rows(o.luma, o.stride);
        in.pw = o.width;
        in.ph = o.height;
        in.x = j.x;
        in.y = j.y;
        in.uxn = j.w >> 2;
        const int units = (j.w >> 2) * (j.h >> 2);
        in.units = units;
        const bool had = a.use_hadamard && !(j.flags & FME_PE_LOSSLESS);
        in.mode = dist_mode(had, j.w, j.h);
        lanes = group_lanes(units);
      }
    }
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
  }
  __syncthreads();
  const int total = total_lanes;
  for (int g0 = 0; g0 < total; g0 += kPeBlock) {   // workgroup-uniform
    const int g = g0 + t;
    const bool act = g < total;
    const int q = act ? (int)slot_task[g >> 2] : 0;
    const PeInfo& in = info[q];
    const int G = act ? in.lanes : 64;
    const int li = g - in.start;
    uint32_t acc = 0;
    if (act) {
      const int mode = in.mode, units = in.units, uxn = in.uxn;
      // the lanes of a quad (4 consecutive lanes) share a task and, with 8x8 Hadamards (units a
      // multiple of 4), run the same iterations: the quad's cross-lane stages see all four lanes
      for (int u = li; u < units; u += G) {
        int ux, uy;
        unit_xy(u, uxn, mode == kDistHad8, ux, uy);
        const int x = in.x + 4 * ux, y = in.y + 4 * uy;
        int p[4][4], d[4][4];
        pe_predict<k10>(in, x, y, p);
        pe_diff<k10>(in, x, y, p, d);
        acc += unit_dist(d, mode, lane, (u & 3) == 0);
      }
    }
    acc = group_sum(acc, G, lane);
    if (act && li == 0) a.dist[t0 + q] = acc >> (k10 ? a.bit_depth - 8 : 0);
  }
}

}  // namespace

hipError_t launch_pred_err(const PeArgs& a, hipStream_t s) {
  return launch_by_depth(k_pred_err<false>, k_pred_err<true>, (a.n + kPeTasks - 1) / kPeTasks, kPeBlock, a, s);
}

}  // namespace fme
