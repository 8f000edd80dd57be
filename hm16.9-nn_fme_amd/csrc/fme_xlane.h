// fme_xlane.h — cross-lane helpers: values of lane ^ m without the LDS pipe, Walsh-Hadamard
// butterflies and sums across a wave (the pixel-per-lane kernels fme_server.hip and fme_px.hip, and
// the unit-per-lane kernels), and the lane groups, unit order and 4x4 Hadamard of the unit-per-lane
// kernels (fme_merge.hip, fme_skip.hip, fme_surface.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fme {
namespace xlane {

// The value of lane ^ m (m a power of two below 64): DPP within a row of 16 lanes,
// v_permlane16/32_swap across rows.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int M>
__device__ __forceinline__ int xor_lane(int v, int lane) {
  if constexpr (M == 1) return dpp_i<0xB1>(v);          // quad_perm [1, 0, 3, 2]
  else if constexpr (M == 2) return dpp_i<0x4E>(v);     // quad_perm [2, 3, 0, 1]
  else if constexpr (M == 4) {                          // row_shl:4 / row_shr:4
    const int up = dpp_i<0x104>(v), dn = dpp_i<0x114>(v);
    return (lane & 4) ? dn : up;
  } else if constexpr (M == 8) return dpp_i<0x128>(v);  // row_ror:8
  else if constexpr (M == 16) {
    const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane & 16) ? (int)p[0] : (int)p[1];
  } else {
    const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (lane & 32) ? (int)p[0] : (int)p[1];
  }
}
// Butterfly stage over lane bit M: (a + b, a - b) with a the lower lane's value.
template <int M>
__device__ __forceinline__ int bfly(int d, int lane) {
  const int p = xor_lane<M>(d, lane);
  return (lane & M) ? p - d : d + p;
}
template <int M>
__device__ __forceinline__ uint32_t xsum(uint32_t a, int lane) { return a + (uint32_t)xor_lane<M>((int)a, lane); }
// sum over all 64 lanes (every lane ends with the total)
__device__ __forceinline__ uint32_t wave_sum(uint32_t a, int lane) {
  return xsum<32>(xsum<16>(xsum<8>(xsum<4>(xsum<2>(xsum<1>(a, lane), lane), lane), lane), lane), lane);
}

// ---- lane groups of the unit-per-lane kernels (k_pred_err, k_pred_sse, k_cost_surface) -----------
// One lane per 4x4 unit.  A task's lane group is its unit count rounded up to a power of two between
// 4 and 64 (a PU of more than 64 units walks them in steps of 64).  A workgroup takes 64 consecutive
// tasks, one per lane of its first wave, and packs their groups into its lanes largest class first:
// every group starts at a multiple of its size and never straddles a wave.
constexpr int kGroupTasks = 64;
constexpr int kGroupSlots = kGroupTasks * 64 / 4;   // 4-lane slots a workgroup's tasks can take

__device__ __forceinline__ int group_lanes(int units) {
  int lanes = 4;
  while (lanes < units && lanes < 64) lanes <<= 1;
  return lanes;
}
// Called by every lane of the first wave with its task's group size (0: no work): writes the task of
// each 4-lane slot and the lanes taken in all, returns the group's first lane slot.
__device__ __forceinline__ int pack_groups(int lanes, int lane, uint8_t (&slot_task)[kGroupSlots], int& total_lanes) {
  int base = 0, start = 0;
#pragma unroll
  for (int c = 64; c >= 4; c >>= 1) {
    const unsigned long long m = __ballot(lanes == c);
    if (lanes == c) start = base + c * __popcll(m & ((1ull << lane) - 1ull));
    base += c * __popcll(m);
  }
  for (int i = 0; i < (lanes >> 2); i++) slot_task[(start >> 2) + i] = (uint8_t)lane;
  if (lane == 0) total_lanes = base;
  return start;
}
// acc summed over the lane group of G lanes (every lane of the wave is here; idle lanes add 0)
__device__ __forceinline__ uint32_t group_sum(uint32_t acc, int G, int lane) {
  { const uint32_t v = (uint32_t)xor_lane<1>((int)acc, lane); acc += v; }
  { const uint32_t v = (uint32_t)xor_lane<2>((int)acc, lane); acc += v; }
  { const uint32_t v = (uint32_t)xor_lane<4>((int)acc, lane); if (G > 4) acc += v; }
  { const uint32_t v = (uint32_t)xor_lane<8>((int)acc, lane); if (G > 8) acc += v; }
  { const uint32_t v = (uint32_t)xor_lane<16>((int)acc, lane); if (G > 16) acc += v; }
  { const uint32_t v = (uint32_t)xor_lane<32>((int)acc, lane); if (G > 32) acc += v; }
  return acc;
}
// (ux, uy) of unit u in a PU of uxn units per row: raster order, or for 8x8 Hadamards the four
// quadrants of an 8x8 block in four consecutive lanes, so that two butterfly stages over the quad
// (bfly<1>, bfly<2>) join their 4x4 transforms.
__device__ __forceinline__ void unit_xy(int u, int uxn, bool quads, int& ux, int& uy) {
  if (quads) {
    const int bxn = max(uxn >> 1, 1), b = u >> 2;
    ux = 2 * (b % bxn) + (u & 1);
    uy = 2 * (b / bxn) + ((u >> 1) & 1);
  } else {
    ux = u % uxn;
    uy = u / uxn;
  }
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

// A PU's distortion per 4x4 unit: the SAD, or with Hadamards xGetHADs' tiles (TComRdCost.cpp:1428-1494):
// 8x8 ((sum |coef| + 2) >> 2 each) when w and h are multiples of 8, else 4x4 ((sum |coef| + 1) >> 1).
enum { kDistSad = 0, kDistHad4 = 1, kDistHad8 = 2 };
__device__ __forceinline__ int dist_mode(bool hadamard, int w, int h) {
  return !hadamard ? kDistSad : ((w | h) & 7) ? kDistHad4 : kDistHad8;
}
// The share of the unit's difference d (transformed in place) in its PU's distortion.  kDistHad8:
// the four lanes of a quad hold the quadrants of one tile (unit_xy) and are all here; two butterfly
// stages over the quad turn their transforms TA, TB, TC, TD into the 8x8 coefficients
// TA +- TB +- TC +- TD, and the tile's value goes to its first lane (lead8), 0 to the others.
__device__ __forceinline__ uint32_t unit_dist(int (&d)[4][4], int mode, int lane, bool lead8) {
  uint32_t s = 0;
  if (mode == kDistSad) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) s += (uint32_t)abs(d[r][c]);
    return s;
  }
  had4x4(d);
  if (mode == kDistHad4) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) s += (uint32_t)abs(d[r][c]);
    return (s + 1) >> 1;
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) s += (uint32_t)abs(bfly<2>(bfly<1>(d[r][c], lane), lane));
  s = xsum<2>(xsum<1>(s, lane), lane);   // the tile's sum of |coef|, in its four lanes
  return lead8 ? (s + 2) >> 2 : 0u;
}

}  // namespace xlane
}  // namespace fme
