// fme_mc_chroma.h — xPredInterBlk's 4:2:0 chroma path shared by the motion-compensation kernels
// (fme_mc.hip) and the skip-check kernel (fme_skip.hip): the 4-tap eighth-pel taps and one list's
// prediction of a 2x2 Cb or Cr unit, at 8 and 10 bits.  The window, the two-stage filter and their
// derivations are fme_mc_luma.h's (UnitWin<4, 2>, pred10<4, 2>).
#pragma once

#include "fme_mc_luma.h"

namespace fme {
namespace mcl {

// TComInterpolationFilter.cpp:65-75 (m_chromaFilter) as int8 quads; fraction 0 is the identity.
__device__ __forceinline__ uint32_t chroma_taps(int f) {
  switch (f) {
    case 0: return q8(0, 64, 0, 0);
    case 1: return q8(-2, 58, 10, -2);
    case 2: return q8(-4, 54, 16, -2);
    case 3: return q8(-6, 46, 28, -4);
    case 4: return q8(-4, 36, 36, -4);
    case 5: return q8(-4, 28, 46, -6);
    case 6: return q8(-2, 16, 54, -4);
    default: return q8(-2, 10, 58, -2);
  }
}

// One list's prediction of the 2x2 unit of component comp (1 Cb, 2 Cr) at chroma position (bx, by)
// (integer MV applied) with the eighth-pel fractions (fx, fy).  (The depth dispatch stands here and
// not behind unit_pred: through that extra layer k_pred_sse<false> allocates 169 VGPRs instead of
// 168 and loses its third wave per SIMD.)
template <bool k10>
__device__ __forceinline__ void chroma_pred(const PicDesc& p, int comp, int bx, int by, int fx, int fy, bool uni,
                                            int (&o)[2][2]) {
  const Plane pl{comp == 1 ? p.cb : p.cr, p.cstride, p.width >> 1, p.height >> 1};
  if constexpr (k10) {
    pred10<4, 2>(pl, bx, by, chroma_taps(fx), 0u, chroma_taps(fy), 0u, uni, o);
  } else {
    UnitWin<4, 2> w;
    w.load(pl, ((p.cstride | (int)(uintptr_t)pl.p) & 3) == 0, bx, by);
    w.pred(chroma_taps(fx), 0u, chroma_taps(fy), 0u, uni, o);
  }
}
// One list's prediction of the 2x2 unit of component comp at chroma position (x, y).
template <bool k10>
__device__ __forceinline__ void list_chroma(const ListMotion& m, int comp, int x, int y, bool uni, int (&o)[2][2]) {
  chroma_pred<k10>(m.pic, comp, x + m.cix, y + m.ciy, m.cfx, m.cfy, uni, o);
}

}  // namespace mcl
}  // namespace fme
