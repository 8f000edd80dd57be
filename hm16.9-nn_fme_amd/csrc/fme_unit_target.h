// fme_unit_target.h — the 4x4 block a unit's sub-pel prediction is compared against, shared by the
// unit-per-lane kernels that price FracDIF positions (fme_surface.hip, fme_direct.hip): the job's
// int16 key block, or the original picture at either bit depth.
#pragma once

#include <hip/hip_runtime.h>

#include "fme_mc_luma.h"
#include "fme_simd.h"

namespace fme {

typedef __attribute__((address_space(1))) const int16_t g_sf_i16;

// o = the 4x4 block the unit at (x, y) is compared against: the job's key block or the original
// (inside it: the job was validated).  Info: the kernel's per-job state with key (the job's key
// block, rows of w, or null), org / ostride / oal (the original, its dword-aligned rows) and the
// PU's x, y, w.
template <bool k10, class Info>
__device__ __forceinline__ void unit_target(const Info& in, int x, int y, bool valid, int (&o)[4][4]) {
  using namespace simd;
  using mcl::gu16c;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) o[r][c] = 0;
  if (!valid) return;
  if (in.key) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      g_sf_i16* kp = (g_sf_i16*)(in.key + (size_t)(y - in.y + r) * in.w + (x - in.x));
#pragma unroll
      for (int c = 0; c < 4; c++) o[r][c] = (int)kp[c];
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if constexpr (k10) {
      const gu16c* op = (const gu16c*)(reinterpret_cast<const uint16_t*>(in.org) + (size_t)(y + r) * in.ostride + x);
#pragma unroll
      for (int c = 0; c < 4; c++) o[r][c] = (int)op[c];
    } else {
      const uint8_t* op = in.org + (size_t)(y + r) * in.ostride + x;
      if (in.oal) {   // x is a multiple of 4
        const uint32_t v = gld32(op);
#pragma unroll
        for (int c = 0; c < 4; c++) o[r][c] = (int)((v >> (8 * c)) & 255u);
      } else {
#pragma unroll
        for (int c = 0; c < 4; c++) o[r][c] = (int)gld8(op + c);
      }
    }
  }
}

}  // namespace fme
