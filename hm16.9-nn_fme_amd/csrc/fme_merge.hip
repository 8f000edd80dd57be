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
constexpr int kPeTasks = 64;   // consecutive tasks per workgroup, set up by its first wave
enum { kPeSad = 0, kPeHad4 = 1, kPeHad8 = 2 };

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
  if (t.w < 4 || t.h < 4 || t.w > 64 || t.h > 64 || (t.w & 3) || (t.h & 3)) return false;
  if (!(t.flags & (FME_MC_L0 | FME_MC_L1)) || (t.flags & ~(FME_MC_L0 | FME_MC_L1 | FME_PE_LOSSLESS))) return false;
  if (t.org_id >= FME_MAX_PICTURES) return false;
  const PicDesc& o = a.pics[t.org_id];
  if (!o.luma || (int)t.x + t.w > o.width || (int)t.y + t.h > o.height) return false;
  for (int l = 0; l < 2; l++) {
    if (!(t.flags & (1u << l))) continue;
    if (t.ref_id[l] >= FME_MAX_PICTURES) return false;
    const PicDesc& p = a.pics[t.ref_id[l]];
    if (!p.luma || p.width != o.width || p.height != o.height) return false;
  }
  return true;
}

// Unnormalised 2-D 4x4 Hadamard in place (rows, then columns).
__device__ __forceinline__ void had4x4(int (&d)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int a = d[r][0] + d[r][1], b = d[r][0] - d[r][1], c = d[r][2] + d[r][3], e = d[r][2] - d[r][3];
    d[r][0] = a + c; d[r][1] = b + e; d[r][2] = a - c; d[r][3] = b - e;
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int a = d[0][c] + d[1][c], b = d[0][c] - d[1][c], e = d[2][c] + d[3][c], f = d[2][c] - d[3][c];
    d[0][c] = a + e; d[1][c] = b + f; d[2][c] = a - e; d[3][c] = b - f;
  }
}

// The prediction of the 4x4 unit at (x, y): both lists in registers, averaged (k_mc's luma block).
template <bool k10>
__device__ __forceinline__ void pe_predict(const PeInfo& in, int x, int y, int (&p)[4][4]) {
  const bool uni = in.nl == 1;
  int o[4][4];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (k >= in.nl) break;
    uint32_t hlo, hhi, vlo, vhi;
    luma_taps(in.fx[k], hlo, hhi);
    luma_taps(in.fy[k], vlo, vhi);
    if constexpr (k10) {
      pred10<8, 4>(Plane16{reinterpret_cast<const uint16_t*>(in.ref[k]), in.rstride[k], in.pw, in.ph}, x + in.ix[k],
                   y + in.iy[k], hlo, hhi, vlo, vhi, uni, o);
    } else {
      UnitWin<8, 4> w;
      w.load(Plane{in.ref[k], in.rstride[k], in.pw, in.ph}, in.ral[k] != 0, x + in.ix[k], y + in.iy[k]);
      w.pred(hlo, hhi, vlo, vhi, uni, o);
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if constexpr (k10) p[r][c] = k == 0 ? o[r][c] : clamp_i((p[r][c] + o[r][c] + 16400) >> 5, 0, 1023);
        else p[r][c] = k == 0 ? o[r][c] : clamp_i((p[r][c] + o[r][c] + 16448) >> 7, 0, 255);
      }
  }
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
  __shared__ uint8_t slot_task[kPeTasks * 64 / 4];   // task of each 4-lane slot
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
        int nl = 0, lists[2] = {0, 0};
        if (j.flags & FME_MC_L0) lists[nl++] = 0;
        if (j.flags & FME_MC_L1) lists[nl++] = 1;
        if (nl == 2 && j.ref_id[0] == j.ref_id[1] && j.mv[0][0] == j.mv[1][0] && j.mv[0][1] == j.mv[1][1])
          nl = 1;   // xCheckIdenticalMotion: same picture, same MV -> xPredInterUni(REF_PIC_LIST_0)
        in.nl = nl;
        const PicDesc o = a.pics[j.org_id];
        for (int k = 0; k < nl; k++) {
          const int l = lists[k];
          const PicDesc p = a.pics[j.ref_id[l]];
          int mx = j.mv[l][0], my = j.mv[l][1];
          clip_mv(mx, my, p.width, p.height, j.cu_x, j.cu_y);
          in.ix[k] = mx >> 2;
          in.iy[k] = my >> 2;
          in.fx[k] = mx & 3;
          in.fy[k] = my & 3;
          in.ref[k] = p.luma;
          in.rstride[k] = p.stride;
          in.ral[k] = ((p.stride | (int)(uintptr_t)p.luma) & 3) == 0;
        }
        in.org = o.luma;
        in.ostride = o.stride;
        in.oal = ((o.stride | (int)(uintptr_t)o.luma) & 3) == 0;
        in.pw = o.width;
        in.ph = o.height;
        in.x = j.x;
        in.y = j.y;
        in.uxn = j.w >> 2;
        const int units = (j.w >> 2) * (j.h >> 2);
        in.units = units;
        const bool had = a.use_hadamard && !(j.flags & FME_PE_LOSSLESS);
        in.mode = !had ? kPeSad : ((j.w | j.h) & 7) ? kPeHad4 : kPeHad8;
        lanes = 4;
        while (lanes < units && lanes < 64) lanes <<= 1;
      }
    }
    // pack the groups by size class, largest first: every start is a multiple of its group size
    int base = 0, start = 0;
#pragma unroll
    for (int c = 64; c >= 4; c >>= 1) {
      const unsigned long long m = __ballot(lanes == c);
      if (lanes == c) start = base + c * __popcll(m & ((1ull << lane) - 1ull));
      base += c * __popcll(m);
    }
    in.lanes = lanes;
    in.start = start;
    for (int i = 0; i < (lanes >> 2); i++) slot_task[(start >> 2) + i] = (uint8_t)t;
    if (t == 0) total_lanes = base;
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
        if (mode == kPeHad8) {   // quadrants of one 8x8 block in consecutive lanes
          const int bxn = uxn >> 1, b = u >> 2;
          ux = 2 * (b % bxn) + (u & 1);
          uy = 2 * (b / bxn) + ((u >> 1) & 1);
        } else {
          ux = u % uxn;
          uy = u / uxn;
        }
        const int x = in.x + 4 * ux, y = in.y + 4 * uy;
        int p[4][4], d[4][4];
        pe_predict<k10>(in, x, y, p);
        pe_diff<k10>(in, x, y, p, d);
        uint32_t s = 0;
        if (mode == kPeSad) {
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) s += (uint32_t)abs(d[r][c]);
          acc += s;
        } else {
          had4x4(d);
          if (mode == kPeHad4) {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
              for (int c = 0; c < 4; c++) s += (uint32_t)abs(d[r][c]);
            acc += (s + 1) >> 1;
          } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
              for (int c = 0; c < 4; c++) s += (uint32_t)abs(bfly<2>(bfly<1>(d[r][c], lane), lane));
            s = xsum<2>(xsum<1>(s, lane), lane);   // the 8x8 block's sum of |coef|, in its four lanes
            if ((u & 3) == 0) acc += (s + 2) >> 2;
          }
        }
      }
    }
    // group sum (every lane of the workgroup is here; idle lanes add 0)
    { const uint32_t v = (uint32_t)xor_lane<1>((int)acc, lane); acc += v; }
    { const uint32_t v = (uint32_t)xor_lane<2>((int)acc, lane); acc += v; }
    { const uint32_t v = (uint32_t)xor_lane<4>((int)acc, lane); if (G > 4) acc += v; }
    { const uint32_t v = (uint32_t)xor_lane<8>((int)acc, lane); if (G > 8) acc += v; }
    { const uint32_t v = (uint32_t)xor_lane<16>((int)acc, lane); if (G > 16) acc += v; }
    { const uint32_t v = (uint32_t)xor_lane<32>((int)acc, lane); if (G > 32) acc += v; }
    if (act && li == 0) a.dist[t0 + q] = acc >> (k10 ? a.bit_depth - 8 : 0);
  }
}

}  // namespace

hipError_t launch_pred_err(const PeArgs& a, hipStream_t s) {
  const dim3 g((a.n + kPeTasks - 1) / kPeTasks);
  if (a.n > 0 && a.bit_depth > 8) hipLaunchKernelGGL(k_pred_err<true>, g, dim3(kPeBlock), 0, s, a);
  else if (a.n > 0) hipLaunchKernelGGL(k_pred_err<false>, g, dim3(kPeBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace fme
