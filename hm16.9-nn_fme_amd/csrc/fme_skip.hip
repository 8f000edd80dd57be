// fme_skip.hip — the skip pass of TEncCu::xCheckRDCostMerge2Nx2N on the GPU (gfx950): the Y, Cb and
// Cr prediction of a block's motion and the three SSEs against the original, fused, with no
// prediction plane written.
//
// One task = motionCompensation (TComPrediction.cpp:495-560) of one block and one motion, then
// TComRdCost::getDistPart(DF_SSE) per component (TComRdCost.cpp:327-345):
//   * prediction: k_mc's path without weighted prediction (fme_mc_luma.h, fme_mc_chroma.h): clipMv
//     per list, xCheckIdenticalMotion, xPredInterBlk per component (luma 8-tap, mv >> 2, mv & 3;
//     4:2:0 chroma 4-tap, mv >> 3, mv & 7), uni clipped to the bit depth, bi through the 14-bit
//     values and TComYuv::addAvg;
//   * distortion: xGetSSE / xGetSSE4..64 (TComRdCost.cpp:861-1205): every width variant is the full
//     sum of (org - pred)^2 >> ((bitDepth - 8) << 1), the shift applied to each sample's square
//     (uiShift = DISTORTION_PRECISION_ADJUSTMENT((bitDepth - 8) << 1)), in UInt.
// The chroma weighting, the cost and the choice are the host's (fme_skip_host.h).
//
// Lanes: k_pred_err's scheme (fme_merge.hip).  One lane per 4x4 luma unit, which also owns the
// co-sited 2x2 Cb and 2x2 Cr units as in k_mc's loop; a task's lane group is its unit count rounded
// up to a power of two between 4 and 64 (a block of more than 64 units walks them in steps of 64);
// a workgroup takes 64 consecutive tasks and packs their groups largest class first, so every
// group starts at a multiple of its size and never straddles a wave.  Three integer accumulators
// per lane, summed over the group by cross-lane adds; the group's first lane writes three dwords.
// Integer arithmetic throughout: a 64x64 block's 8-bit sum reaches 4096 * 255^2 < 2^32, and at 10
// bits each term is (1023^2) >> 4 = 65408, so 4096 terms stay below 2^32 too.
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_mc_chroma.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"
#include "fme_xlane.h"

namespace fme {
namespace {

using namespace simd;
using namespace mcl;
using namespace xlane;

constexpr int kSseBlock = 256;
constexpr int kSseTasks = kGroupTasks;   // consecutive tasks per workgroup, set up by its first wave

// Per-task state shared by the workgroup (LDS), filled by one thread per task.
struct SseInfo {
  PicDesc ref[2];             // the predicted lists' pictures
  PicDesc org;
  int x, y, uxn, units;
  int lanes, start;           // lane group size (0: no work) and first lane slot
  int nl;                     // lists predicted (2: bi)
  int lix[2], liy[2], lfx[2], lfy[2];   // luma integer offsets / quarter-pel fractions per list
  int cix[2], ciy[2], cfx[2], cfy[2];   // chroma (eighth-pel) per list
};

__device__ __forceinline__ bool sse_task_valid(const SseArgs& a, const fme_sse_task& t) {
  if (!pu_shape_ok(t.w, t.h)) return false;
  if (!(t.flags & (FME_MC_L0 | FME_MC_L1)) || (t.flags & ~(FME_MC_L0 | FME_MC_L1))) return false;
  if (t.org_id >= FME_MAX_PICTURES) return false;
  const PicDesc& o = a.pics[t.org_id];
  if (!o.luma || !o.cb || !o.cr || (int)t.x + t.w > o.width || (int)t.y + t.h > o.height) return false;
  return refs_ok(t.flags, t.ref_id, a.pics, o.width, o.height, true);
}

// (org - pred)^2 >> ((bitDepth - 8) << 1) of one sample
template <bool k10>
__device__ __forceinline__ uint32_t sq(int org, int pred, int shift) {
  const int d = org - pred;
  const uint32_t s = (uint32_t)(d * d);
  return k10 ? s >> shift : s;
}

// The SSE of the 4x4 luma unit at (x, y) (inside the original: the task was validated).
template <bool k10>
__device__ __forceinline__ uint32_t sse_luma(const SseInfo& in, int x, int y, int shift) {
  const bool uni = in.nl == 1;
  int p[4][4];
  pred_lists<k10>(in.nl, [&](int k, int (&o)[4][4]) {
    const PicDesc& r = in.ref[k];
    luma_pred<k10>(luma_plane(r), dword_rows(r.luma, r.stride), x + in.lix[k], y + in.liy[k], in.lfx[k], in.lfy[k], uni,
                   o);
  }, p);
  uint32_t s = 0;
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    const size_t row = (size_t)(y + rr) * in.org.stride + x;
#pragma unroll
    for (int c = 0; c < 4; c++) s += sq<k10>(ld_sample<k10>(in.org.luma, row + c), p[rr][c], shift);
  }
  return s;
}

// The SSE of the 2x2 unit of component comp (1 Cb, 2 Cr) at chroma position (x, y).
template <bool k10>
__device__ __forceinline__ uint32_t sse_chroma(const SseInfo& in, int comp, int x, int y, int shift) {
  const bool uni = in.nl == 1;
  int p[2][2];
  pred_lists<k10>(in.nl, [&](int k, int (&o)[2][2]) {
    chroma_pred<k10>(in.ref[k], comp, x + in.cix[k], y + in.ciy[k], in.cfx[k], in.cfy[k], uni, o);
  }, p);
  const uint8_t* plane = comp == 1 ? in.org.cb : in.org.cr;
  uint32_t s = 0;
#pragma unroll
  for (int rr = 0; rr < 2; rr++) {
    const size_t row = (size_t)(y + rr) * in.org.cstride + x;
#pragma unroll
    for (int c = 0; c < 2; c++) s += sq<k10>(ld_sample<k10>(plane, row + c), p[rr][c], shift);
  }
  return s;
}

template <bool k10>
__global__ __launch_bounds__(kSseBlock) void k_pred_sse(SseArgs a) {
  __shared__ SseInfo info[kSseTasks];
  __shared__ uint8_t slot_task[kGroupSlots];   // task of each 4-lane slot
  __shared__ int total_lanes;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kSseTasks;
  if (t < kSseTasks) {   // the first wave: one task per lane
    SseInfo& in = info[t];
    int lanes = 0;
    const int ti = t0 + t;
    if (ti < a.n) {
      const fme_sse_task j = a.tasks[ti];
      if (!sse_task_valid(a, j)) {
        atomicAdd(a.invalid, 1);
        a.sse[3 * (size_t)ti + 0] = 0xFFFFFFFFu;
        a.sse[3 * (size_t)ti + 1] = 0xFFFFFFFFu;
        a.sse[3 * (size_t)ti + 2] = 0xFFFFFFFFu;
      } else {
        // resolve_lists' text (fme_mc_luma.h), kept local: with ListMotion in SseInfo the 8-bit kernel
        // allocates 169 VGPRs instead of 168 and loses its third wave per SIMD, and a local
        // ListMotion copied into these fields goes to scratch
        int nl = ((j.flags & FME_MC_L0) ? 1 : 0) + ((j.flags & FME_MC_L1) ? 1 : 0);
        if (nl == 2 && j.ref_id[0] == j.ref_id[1] && j.mv[0][0] == j.mv[1][0] && j.mv[0][1] == j.mv[1][1])
          nl = 1;   // xCheckIdenticalMotion: same picture, same MV -> xPredInterUni(REF_PIC_LIST_0)
        in.nl = nl;
#pragma unroll
        for (int k = 0; k < 2; k++) {   // (selects, not indexed reads: the task stays in registers)
          if (k >= nl) break;
          const bool l1 = k == 1 || !(j.flags & FME_MC_L0);   // the k-th predicted list is list 1
          const PicDesc p = a.pics[l1 ? j.ref_id[1] : j.ref_id[0]];
          int mx = l1 ? j.mv[1][0] : j.mv[0][0], my = l1 ? j.mv[1][1] : j.mv[0][1];
          clip_mv(mx, my, p.width, p.height, j.cu_x, j.cu_y);
          in.lix[k] = mx >> 2;   // xPredInterBlk: shift 2 + csx, fraction mask (4 << csx) - 1
          in.liy[k] = my >> 2;
          in.lfx[k] = mx & 3;
          in.lfy[k] = my & 3;
          in.cix[k] = mx >> 3;
          in.ciy[k] = my >> 3;
          in.cfx[k] = mx & 7;
          in.cfy[k] = my & 7;
          in.ref[k] = p;
        }
        in.org = a.pics[j.org_id];
        in.x = j.x;
        in.y = j.y;
        in.uxn = j.w >> 2;
        const int units = (j.w >> 2) * (j.h >> 2);
        in.units = units;
        lanes = group_lanes(units);
      }
    }
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
  }
  __syncthreads();
  const int total = total_lanes;
  const int shift = k10 ? (a.bit_depth - 8) << 1 : 0;
  for (int g0 = 0; g0 < total; g0 += kSseBlock) {   // workgroup-uniform
    const int g = g0 + t;
    const bool act = g < total;
    const int q = act ? (int)slot_task[g >> 2] : 0;
    const SseInfo& in = info[q];
    const int G = act ? in.lanes : 64;
    const int li = g - in.start;
    uint32_t ay = 0, acb = 0, acr = 0;
    if (act) {
      const int units = in.units, uxn = in.uxn;
      for (int u = li; u < units; u += G) {
        const int ux = u % uxn, uy = u / uxn;
        ay += sse_luma<k10>(in, in.x + 4 * ux, in.y + 4 * uy, shift);
        const int cx = (in.x >> 1) + 2 * ux, cy = (in.y >> 1) + 2 * uy;
        acb += sse_chroma<k10>(in, 1, cx, cy, shift);
        acr += sse_chroma<k10>(in, 2, cx, cy, shift);
      }
    }
    ay = group_sum(ay, G, lane);
    acb = group_sum(acb, G, lane);
    acr = group_sum(acr, G, lane);
    if (act && li == 0) {
      uint32_t* out = a.sse + 3 * (size_t)(t0 + q);
      out[0] = ay;
      out[1] = acb;
      out[2] = acr;
    }
  }
}

}  // namespace

hipError_t launch_pred_sse(const SseArgs& a, hipStream_t s) {
  return launch_by_depth(k_pred_sse<false>, k_pred_sse<true>, (a.n + kSseTasks - 1) / kSseTasks, kSseBlock, a, s);
}

}  // namespace fme
