// fme_lane_common.h — the skeleton the lane-per-unit search kernels of both bit depths share
// (fme_lane.hip: 8 bits, samples as bytes; fme_lane10.hip: 10 bits, samples as int16): the class
// table, the small helpers, the LDS tables, the lane-to-unit mapping, the sums over a PU's lanes,
// the candidate bookkeeping, and the workgroup's table fill and claim loop.
//
// What depends on the sample format stays in the two files: window and key loads, the nine EMI
// distortions, the filters and the unit's distortion.  So do three pieces that are the same in
// both but change the per-class functions' code when they become functions here:
// the EMI square-step decision, the pass over a two-unit lane's halves, and the record staging
// and store (which use g_rec / g_rec_jid below).
//
// Included once by each of the two files, which compile to separate code objects: each gets its own
// copy of the LDS tables below.  Everything here is inlined into the per-class functions (or the
// kernel); those stay one noinline function per class in each file.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "fme_device.h"
#include "fme_simd.h"

// (class id, PU W, PU H, unit W, unit H) of every class (fme_device.h class table), in the order
// the per-class functions are emitted.  4x8 units for every shape whose width is a multiple of 4 and
// height a multiple of 8 (an 8x8 SATD tile is a lane pair; the 4x4-tiled 4x8 / 4x16 / 12x16 keep
// their two tiles in the lane), 4x4 units (one SATD tile each) for 8x4 / 16x4 / 16x12.  (4x4 units
// for 4x8-tiled shapes: about 18 % more instructions per PU, measured 0.924 -> 0.9xx ms; 8x4 units
// for the 8x4-like shapes gave wrong half / quarter results on ~15 % of their golden jobs and are
// not used)  The AMP shapes' unit counts are not powers of two: 12x16 (6 of 8
// lanes), 16x12 (12 of 16), 24x32 / 32x24 (24 of 32), 48x64 / 64x48 (two halves of 48 units, 48 of
// 64 lanes).
#ifndef FME_LANE_CLASSES   // (a subset may be given on the command line for register-usage probes)
#define FME_LANE_CLASSES(X)                                                                          \
  X(0, 4, 8, 4, 8) X(3, 4, 16, 4, 8) X(1, 8, 4, 4, 4) X(4, 16, 4, 4, 4) X(2, 8, 8, 4, 8)              \
  X(5, 8, 16, 4, 8) X(6, 16, 8, 4, 8) X(9, 16, 16, 4, 8) X(10, 8, 32, 4, 8) X(11, 32, 8, 4, 8)        \
  X(12, 16, 32, 4, 8) X(13, 32, 16, 4, 8) X(16, 32, 32, 4, 8) X(17, 16, 64, 4, 8) X(18, 64, 16, 4, 8) \
  X(19, 32, 64, 4, 8) X(20, 64, 32, 4, 8) X(23, 64, 64, 4, 8) X(7, 12, 16, 4, 8) X(8, 16, 12, 4, 4)   \
  X(14, 24, 32, 4, 8) X(15, 32, 24, 4, 8) X(21, 48, 64, 4, 8) X(22, 64, 48, 4, 8)
#endif

#define FME_AI __attribute__((always_inline))

namespace fme {
namespace {
using namespace simd;

constexpr int kLaneNT = 256;   // threads per workgroup of either kernel: four wave tiles per claim

// ---- small helpers -------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
// Sum over the L lanes of a PU's group (L a power of two <= 64): every lane of the group ends
// with the total.  Offsets 1, 2 swap within a quad (DPP quad_perm); once each quad / octet
// holds its sum, the half-mirror / mirror partner of a lane (DPP row_half_mirror / row_mirror,
// lane i <-> 7-i / 15-i) lies in the other quad / octet; 16 is a ds_swizzle xor, 32 a
// bpermute.  (A/B on the 1080p batch: -1 % search time against bpermute for every step.)
template <int L>
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
  if (L >= 2) v += dpp<0xB1>(v);
  if (L >= 4) v += dpp<0x4E>(v);
  if (L >= 8) v += dpp<0x141>(v);
  if (L >= 16) v += dpp<0x140>(v);
  if (L >= 32) v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
  if (L >= 64) v += (uint32_t)__shfl_xor((int)v, 32, 64);
  return v;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__host__ __device__ __forceinline__ constexpr int pow2_at_least(int v) { return v <= 1 ? 1 : 2 * pow2_at_least((v + 1) / 2); }

// low 16 bits of a and b -> one packed pair (a in the low half)
__device__ __forceinline__ uint32_t pack2(int a, int b) { return __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x05040100u); }

// Opaque to the optimiser (no instructions): values derived from the window before this point
// are not reused after it, so common subexpressions do not stay live across passes.
template <int R, int N>
__device__ __forceinline__ void launder(uint32_t (&v)[R][N]) {
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int k = 0; k < N; k++) asm volatile("" : "+v"(v[r][k]));
}

// The XCD this wave runs on (HW_REG_XCC_ID, gfx940+: bits 3:0).
__device__ __forceinline__ int xcc_id() { return __builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11)) & 7; }

// Global pointers typed as such (global_load / global_store, not flat).
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x3a __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x2a __attribute__((ext_vector_type(2), aligned(4)));
typedef __attribute__((address_space(1))) const u32x4a gu4;
typedef __attribute__((address_space(1))) const u32x3a gu3;
typedef __attribute__((address_space(1))) const u32x2a gu2;
typedef __attribute__((address_space(1))) const int32_t g_i32;
typedef __attribute__((address_space(1))) fme_result g_res;
typedef __attribute__((address_space(1))) const int16_t g_i16;
typedef __attribute__((address_space(1))) const uint32_t g_u32;

// N dwords from byte address p, any alignment (gfx950 runs global memory in unaligned access
// mode; tools/probes/unaligned_probe.hip checks it on the box).
template <int N>
__device__ __forceinline__ void ld_bytes(const void* p, uint32_t (&o)[N]) {
  const uint8_t* q = (const uint8_t*)p;
  constexpr int K4 = N / 4 * 4;
#pragma unroll
  for (int k = 0; k < K4; k += 4) {
    const u32x4a v = *(gu4*)(q + 4 * k);
    o[k] = v.x; o[k + 1] = v.y; o[k + 2] = v.z; o[k + 3] = v.w;
  }
  if constexpr (N - K4 == 3) {
    const u32x3a v = *(gu3*)(q + 4 * K4);
    o[K4] = v.x; o[K4 + 1] = v.y; o[K4 + 2] = v.z;
  } else if constexpr (N - K4 == 2) {
    const u32x2a v = *(gu2*)(q + 4 * K4);
    o[K4] = v.x; o[K4 + 1] = v.y;
  } else if constexpr (N - K4 == 1) {
    o[K4] = gld32(q + 4 * K4);
  }
}

// Candidate offsets (xPatternRefinement tables, TEncSearch.cpp:212-236).
__host__ __device__ __forceinline__ constexpr int h9_dx(int i) { return (i == 3 || i == 5 || i == 7) ? -1 : ((i == 4 || i == 6 || i == 8) ? 1 : 0); }
__host__ __device__ __forceinline__ constexpr int h9_dy(int i) { return (i == 1 || i == 5 || i == 6) ? -1 : ((i == 2 || i == 7 || i == 8) ? 1 : 0); }
__host__ __device__ __forceinline__ constexpr int q9_dx(int i) { return (i == 3 || i == 5 || i == 7) ? -1 : ((i == 4 || i == 6 || i == 8) ? 1 : 0); }
__host__ __device__ __forceinline__ constexpr int q9_dy(int i) { return (i == 1 || i == 3 || i == 4) ? -1 : ((i == 2 || i == 7 || i == 8) ? 1 : 0); }
// Q9 index of (dqx, dqy)
__host__ __device__ __forceinline__ constexpr int q9_index(int dx, int dy) {
  return dy == 0 ? (dx == 0 ? 0 : (dx < 0 ? 5 : 6)) : dy < 0 ? (dx == 0 ? 1 : (dx < 0 ? 3 : 4)) : (dx == 0 ? 2 : (dx < 0 ? 7 : 8));
}
// EMI positions: 0 centre, then TL, T, TR, L, R, BL, B, BR (xTZ8PointSquareSearch order)
__host__ __device__ __forceinline__ constexpr int emi_dx(int p) { return (p == 1 || p == 4 || p == 6) ? -1 : ((p == 3 || p == 5 || p == 8) ? 1 : 0); }
__host__ __device__ __forceinline__ constexpr int emi_dy(int p) { return p >= 1 && p <= 3 ? -1 : (p >= 6 ? 1 : 0); }

// ---- per-workgroup LDS tables ----------------------------------------------------------------
// Per-workgroup copies of the batch's picture and lambda tables (lane_claim_loop fills them once):
// every tile reads its PU's reference / original picture descriptor and motion lambda from LDS
// instead of a dependent global load before its window loads.
__shared__ PicDesc g_pics[FME_MAX_PICTURES];
// MV bits of one candidate: two exp-Golomb lengths of values below 2^18 (int16 MVs and predictors,
// cost scale <= 2), each at most 37.
constexpr int kCostBits = 80;
__shared__ uint32_t g_cost[FME_MAX_LAMBDAS][kCostBits];
// Record staging: each PU's 64-byte fme_result is assembled in LDS by the PU's first lane, then
// the wave writes the tile's records with four lanes per record, so every store instruction writes
// whole 64-byte lines (one lane per record wrote four separate 16-byte pieces: 256 bytes of
// WRITE_SIZE per job).
__shared__ uint4 g_rec[kLaneNT / 64][64][4];
__shared__ int32_t g_rec_jid[kLaneNT / 64][64];

// ---- candidates --------------------------------------------------------------------------------
// The MV cost from the workgroup's table: g_cost[lambda][bits] = (UInt)(mlambda * bits / 65536.0)
// (TComRdCost.h:165), computed once per launch by the same double arithmetic.
__device__ __forceinline__ uint32_t mv_cost(const uint32_t* ml, uint32_t bits) { return ml[bits]; }
// `live`: ~0 on the lanes of a PU's units, 0 on the idle lanes that pad a group of 6 / 12 / 48
// units (AMP shapes) to a power of two, so they add nothing to the group's sum.  DSH:
// DISTORTION_PRECISION_ADJUSTMENT(bitDepth - 8) of the PU's summed SATD / SAD (0 at 8 bits, 2 at 10).
// Candidates arrive out of H9 / Q9 order: the first strict minimum in that order is kept with an
// index tie-break (d < best, or d == best at a lower index).
template <int L, int DSH>
__device__ __forceinline__ void take_half(int i, uint32_t part, uint32_t live, const uint32_t* ml, int mvx, int mvy, int px,
                                          int py, uint32_t& best, int& bi) {
  const uint32_t d = (group_sum<L>(part & live) >> DSH) + mv_cost(ml, mv_bits(2 * mvx + h9_dx(i), 2 * mvy + h9_dy(i), 1, px, py));
  if (d < best || (d == best && i < bi)) {
    best = d;
    bi = i;
  }
}
template <int L, int DSH>
__device__ __forceinline__ void take_qtr(int i, uint32_t part, uint32_t live, const uint32_t* ml, int mvx, int mvy, int hx,
                                         int hy, int px, int py, uint32_t& best, int& bi) {
  const int qx = 2 * hx + q9_dx(i), qy = 2 * hy + q9_dy(i);
  const uint32_t d = (group_sum<L>(part & live) >> DSH) + mv_cost(ml, mv_bits(4 * mvx + qx, 4 * mvy + qy, 0, px, py));
  if (d < best || (d == best && i < bi)) {
    best = d;
    bi = i;
  }
}

// ---- lane -> unit ----------------------------------------------------------------------------
// Lane `lane` of wave tile wt (64 lanes = 64 / L PUs of a class with cnt PUs): PU p of the class,
// unit u of the PU's group of L lanes, NUH of them real units (ux, uy) of a PU UX units wide.
struct LaneMap {
  int lane, p, u, ux, uy;
  bool active;     // false past the class's last PU: duplicate work, no stores (keeps the group whole)
  uint32_t live;   // 0 on the padding lanes, which repeat the last unit and are summed as 0
};
template <int L, int NUH, int UX>
__device__ __forceinline__ LaneMap lane_map(int wt, int cnt) {
  LaneMap m;
  m.lane = (int)__lane_id();
  const int gl = wt * 64 + m.lane;
  m.p = gl / L;
  m.u = gl - m.p * L;
  m.active = m.p < cnt;
  if (!m.active) m.p = cnt - 1;
  m.live = m.u < NUH ? ~0u : 0u;
  const int uu = m.u < NUH ? m.u : NUH - 1;
  m.ux = uu % UX;
  m.uy = uu / UX;
  return m;
}

// ---- the workgroup: table fill and claim loop -----------------------------------------------
// One persistent kernel serves every class.  A workgroup claims four consecutive 64-lane wave tiles
// (one per wave; a tile holds 64 / L PUs of one class) per atomic from its XCD's queue
// (Schedule::xq: the XCD's contiguous eighth of every class's tiles = one spatial band of the
// CTU-ordered job stream, so each L2 sees one band, and the four waves of a CU search neighbouring
// PUs whose reference windows share L1 lines), then from the other XCDs' queues.  The next claim is
// issued before the current tiles are searched.  The grid is sized to fill the chip (lane_grid), not
// to the (device-computed) tile count, so the host never waits for the class histogram.
// Measured (1080p frame, tools/ab_bench.py): per-wave claims 1.48 ms, four tiles per workgroup
// 1.21 ms, eight 1.24, sixteen 1.29; without the XCD queues 1.25 (the per-wave claim form was
// kept as a build option until round 5 and removed unused).
// dispatch(sc, c, wt, wid): wave wid searches wave tile wt of class c.
template <int NT, class F>
__device__ __forceinline__ void lane_claim_loop(const BatchArgs& a, const WorkBufs& w, F&& dispatch) {
  const Schedule* __restrict__ sc = w.sched;
  int32_t* ctr = w.tile_ctr;
  __shared__ int32_t s_xq[8][kNumClasses + 1];
  {   // the batch's tables and the XCD queues, once per workgroup
    const uint32_t* ps = reinterpret_cast<const uint32_t*>(a.pics);
    uint32_t* pd = reinterpret_cast<uint32_t*>(g_pics);
    for (int i = threadIdx.x; i < (int)(sizeof(g_pics) / 4); i += NT) pd[i] = ps[i];
    for (int i = threadIdx.x; i < FME_MAX_LAMBDAS * kCostBits; i += NT)
      g_cost[i / kCostBits][i % kCostBits] = simd::mv_cost(a.mlambda[i / kCostBits], (uint32_t)(i % kCostBits));
    for (int i = threadIdx.x; i < 8 * (kNumClasses + 1); i += NT) (&s_xq[0][0])[i] = (&sc->xq[0][0])[i];
  }
  const int home = xcc_id(), wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  constexpr int kGroup = NT / 64;   // wave tiles per claim
  __shared__ int32_t claim[2];
  int x = home, tried = 0, par = 0;
  if (threadIdx.x == 0) claim[0] = atomicAdd(&ctr[x], 1);
  __syncthreads();
  int t = __builtin_amdgcn_readfirstlane(claim[0]);
  while (true) {
    const int len = s_xq[x][kNumClasses];
    if (kGroup * t >= len) {   // queue drained: the next XCD's
      if (++tried == 8) break;
      x = (home + tried) & 7;
      par ^= 1;
      if (threadIdx.x == 0) claim[par] = atomicAdd(&ctr[x], 1);
      __syncthreads();
      t = __builtin_amdgcn_readfirstlane(claim[par]);
      continue;
    }
    int nxt = 0;
    if (threadIdx.x == 0) nxt = atomicAdd(&ctr[x], 1);
    const int tw = kGroup * t + wid;
    if (tw < len) {
      int c = 0;   // the queue position of tile tw's class
      while (c < kNumClasses - 1 && tw >= s_xq[x][c + 1]) c++;
      const int ci = c;   // queue position -> class
      c = lane_class_at(ci);
      const int nt = sc->prefix[c + 1] - sc->prefix[c];
      const int lo = (int)(((long long)nt * x) / 8);   // the band's first tile of class c
      // wave-uniform: kept in an SGPR, so no VGPR of it lives (and is spilled) across the call
      const int wt = __builtin_amdgcn_readfirstlane(lo + (tw - s_xq[x][ci]));
      dispatch(sc, c, wt, wid);
    }
    par ^= 1;   // claim[par] is rewritten only after every wave has passed the barrier below
    if (threadIdx.x == 0) claim[par] = nxt;
    __syncthreads();
    t = __builtin_amdgcn_readfirstlane(claim[par]);
  }
}

}  // namespace
}  // namespace fme
