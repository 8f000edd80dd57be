// fme_mc_luma.h — xPredInterBlk's building blocks shared by the motion-compensation kernels
// (fme_mc.hip), the prediction-error kernel (fme_merge.hip) and the skip-check kernel (fme_skip.hip):
// the luma interpolation taps, clipMv, the edge-replicated reference window of one output unit and
// its two-stage filter, at 8 and 10 bits.
// The derivations are in fme_mc.hip's module header.
#pragma once

#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_simd.h"

namespace fme {
namespace mcl {

using namespace simd;

// TComInterpolationFilter.cpp:57-63 as int8 quads (taps 0-3, 4-7; the chroma taps: fme_mc_chroma.h).
// Fraction 0 uses the identity filter (64 at the centre tap): through the two-stage form below
// it reproduces filterCopy and the 1-D filters exactly (fme_mc.hip's module header).
__device__ __forceinline__ void luma_taps(int f, uint32_t& lo, uint32_t& hi) {
  lo = f == 0 ? q8(0, 0, 0, 64) : f == 1 ? q8(-1, 4, -10, 58) : f == 2 ? q8(-1, 4, -11, 40) : q8(0, 1, -5, 17);
  hi = f == 0 ? 0u : f == 1 ? q8(17, -5, 1, 0) : f == 2 ? q8(40, -11, 4, -1) : q8(58, -10, 4, -1);
}
__device__ __forceinline__ int tap_of(uint32_t lo, uint32_t hi, int k) {   // signed byte k of (lo, hi)
  const uint32_t w = k < 4 ? lo : hi;
  return (int)(int8_t)(w >> (8 * (k & 3)));
}

typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x3a __attribute__((ext_vector_type(3), aligned(4)));
typedef __attribute__((address_space(1))) const u32x4a gu4;
typedef __attribute__((address_space(1))) const u32x3a gu3;

struct Plane {
  const uint8_t* p;
  int stride, w, h;
};

// TComDataCU::clipMv (TComDataCU.cpp:2773-2786), max CU 64 (sps.getMaxCUWidth/Height)
__device__ __forceinline__ void clip_mv(int& mx, int& my, int pic_w, int pic_h, int cu_x, int cu_y) {
  const int hor_max = (pic_w + 8 - cu_x - 1) << 2, hor_min = (-64 - 8 - cu_x + 1) * 4;
  const int ver_max = (pic_h + 8 - cu_y - 1) << 2, ver_min = (-64 - 8 - cu_y + 1) * 4;
  mx = min(hor_max, max(hor_min, mx));
  my = min(ver_max, max(ver_min, my));
}

// Rows of (s - 128) bytes of a window: R rows from plane row y0, ND dwords from byte x0 & ~3
// (edge-replicated), and the byte shift of x0 inside the first dword.
template <int R, int ND>
__device__ __forceinline__ uint32_t load_window(const Plane& pl, int x0, int y0, bool aligned, uint32_t (&w)[R][ND]) {
  const int xa = x0 & ~3;
  const bool inside = aligned && xa >= 0 && xa + 4 * ND <= pl.w && y0 >= 0 && y0 + R <= pl.h;
  if (inside) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint8_t* row = pl.p + (size_t)(y0 + r) * pl.stride + xa;
      if constexpr (ND == 4) {
        const u32x4a v = *(gu4*)row;
        w[r][0] = v.x ^ 0x80808080u; w[r][1] = v.y ^ 0x80808080u;
        w[r][2] = v.z ^ 0x80808080u; w[r][3] = v.w ^ 0x80808080u;
      } else if constexpr (ND == 3) {
        const u32x3a v = *(gu3*)row;
        w[r][0] = v.x ^ 0x80808080u; w[r][1] = v.y ^ 0x80808080u; w[r][2] = v.z ^ 0x80808080u;
      } else {
#pragma unroll
        for (int k = 0; k < ND; k++) w[r][k] = gld32(row + 4 * k) ^ 0x80808080u;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint8_t* row = pl.p + (size_t)clamp_i(y0 + r, 0, pl.h - 1) * pl.stride;
#pragma unroll
      for (int k = 0; k < ND; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) v |= gld8(row + clamp_i(xa + 4 * k + b, 0, pl.w - 1)) << (8 * b);
        w[r][k] = v ^ 0x80808080u;
      }
    }
  }
  return (uint32_t)(x0 - xa);
}

// One U x U output unit of one list (N taps; U = 4 luma, 2 chroma): its window of R = U + N - 1
// rows of (s - 128) bytes around plane position (bx, by) (integer MV applied).
template <int N, int U>
struct UnitWin {
  static constexpr int R = U + N - 1;                   // window rows and columns
  static constexpr int NA = ((U - 1 + N - 4) >> 2) + 2; // re-aligned dwords the dot4 groups read
  static constexpr int ND = NA + 1;                     // dwords loaded per row (any alignment)
  uint32_t w[R][ND];
  uint32_t s0;
  __device__ __forceinline__ void load(const Plane& pl, bool aligned, int bx, int by) {
    s0 = load_window<R, ND>(pl, bx - (N / 2 - 1), by - (N / 2 - 1), aligned, w);
  }
  // Two stages in the (s - 128) domain, which absorbs filterCopy / filter<N, ., isFirst = true,
  // .>'s -IF_INTERNAL_OFFS: stage 1 = sum c.s - 8192; stage 2 uni (isLast): (sum + 2048 +
  // (8192 << 6)) >> 12 clipped, bi: sum >> 6 (14-bit).
  __device__ __forceinline__ void pred(uint32_t hlo, uint32_t hhi, uint32_t vlo, uint32_t vhi, bool uni,
                                       int (&out)[U][U]) const {
    int t[R][U];
#pragma unroll
    for (int r = 0; r < R; r++) {
      uint32_t a[NA];
#pragma unroll
      for (int k = 0; k < NA; k++) a[k] = __builtin_amdgcn_alignbyte(w[r][k + 1], w[r][k], s0);
#pragma unroll
      for (int c = 0; c < U; c++) {   // bytes c .. c+N-1 of the re-aligned row
        const uint32_t b0 = (c & 3) ? __builtin_amdgcn_alignbyte(a[(c >> 2) + 1], a[c >> 2], (uint32_t)(c & 3)) : a[c >> 2];
        int acc = dot4(b0, hlo, 0);
        if constexpr (N == 8) {
          const int q = c + 4;
          const uint32_t b1 = (q & 3) ? __builtin_amdgcn_alignbyte(a[(q >> 2) + 1], a[q >> 2], (uint32_t)(q & 3)) : a[q >> 2];
          acc = dot4(b1, hhi, acc);
        }
        t[r][c] = acc;
      }
    }
#pragma unroll
    for (int y = 0; y < U; y++)
#pragma unroll
      for (int c = 0; c < U; c++) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < N; k++) sum += t[y + k][c] * tap_of(vlo, vhi, k);
        out[y][c] = uni ? clamp_i((sum + 2048 + (8192 << 6)) >> 12, 0, 255) : (sum >> 6);
      }
  }
};

// ---- bit depth 10 (the main10 configurations): uint16 planes, int samples -----------------------
// xPredInterBlk at bitDepth 10 (headRoom 4, TComInterpolationFilter.cpp:94-257) in the same
// two-stage form as the 8-bit kernel: with s' = s - 512 the first stage filter<N, ., isFirst,
// !isLast> is h = (sum c s - (8192 << 2)) >> 2 = (sum c s') >> 2 (the identity filter gives
// filterCopy's 16 s'), the second uni (isLast): ((sum c h + 512) >> 10) + 512 clipped to 0..1023,
// bi (!isLast): (sum c h) >> 6, which is HM's 14-bit value for every fraction pair (a zero fraction
// is the identity: (64 h) >> 6 = h, (16 sum c s') >> 6 = (sum c s') >> 2).  TComYuv::addAvg at
// bitDepth 10: (p0 + p1 + 16400) >> 5 clipped (shift 14 + 1 - 10, offset 16 + 2 * 8192).
struct Plane16 {
  const uint16_t* p;
  int stride, w, h;
};
typedef __attribute__((address_space(1))) const uint16_t gu16c;

template <int N, int U>
__device__ __forceinline__ void pred10(const Plane16& pl, int bx, int by, uint32_t hlo, uint32_t hhi, uint32_t vlo,
                                       uint32_t vhi, bool uni, int (&out)[U][U]) {
  constexpr int R = U + N - 1;
  const int x0 = bx - (N / 2 - 1), y0 = by - (N / 2 - 1);
  int h[R][U];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const gu16c* row = (const gu16c*)(pl.p + (size_t)clamp_i(y0 + r, 0, pl.h - 1) * pl.stride);
    int sv[R];
#pragma unroll
    for (int c = 0; c < R; c++) sv[c] = (int)row[clamp_i(x0 + c, 0, pl.w - 1)] - 512;
#pragma unroll
    for (int c = 0; c < U; c++) {
      int acc = 0;
#pragma unroll
      for (int k = 0; k < N; k++) acc += tap_of(hlo, hhi, k) * sv[c + k];
      h[r][c] = acc >> 2;
    }
  }
#pragma unroll
  for (int y = 0; y < U; y++)
#pragma unroll
    for (int c = 0; c < U; c++) {
      int sum = 0;
#pragma unroll
      for (int k = 0; k < N; k++) sum += h[y + k][c] * tap_of(vlo, vhi, k);
      out[y][c] = uni ? clamp_i(((sum + 512) >> 10) + 512, 0, 1023) : (sum >> 6);
    }
}

}  // namespace mcl
}  // namespace fme
