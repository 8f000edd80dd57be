// fme_direct_host.h — the arithmetic of the NN-direct path (include/fme_direct.h) that needs no GPU:
// how an NN_pred() class splits into the position the evaluation predicts at and into the four
// globals MVX_HALF, MVX_QRTER, MVY_HALF, MVY_QRTER, and the argument checks of the entry points.
// Plain C++ over include/fme_direct.h: no HIP, so a CPU test can include it alone
// (tests/cpp/test_direct_host.cpp); the kernel (fme_direct.hip) and the runtime include it too, hence
// FME_DIRECT_HD.
#pragma once

#include <cstdint>

#include "../../include/fme_direct.h"

#if defined(__HIPCC__)
#define FME_DIRECT_HD __host__ __device__ inline
#else
#define FME_DIRECT_HD inline
#endif

namespace fme {

static_assert((FME_RES_NN_DIRECT & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_REJECTED)) == 0,
              "FME_RES_NN_DIRECT is a status bit of its own");

constexpr int kDirectClasses = 49;

// Quarter-pel offset of a class, each component in -3..3 (TEncSearch.cpp:4590-4591 applies
// 2 half + quarter of the class's globals, which is this offset).
FME_DIRECT_HD int direct_dx(int cls) { return cls % 7 - 3; }
FME_DIRECT_HD int direct_dy(int cls) { return cls / 7 - 3; }

// One component o in -3..3 as the switch at TEncSearch.cpp:136-193 splits it: o = 2 half + quarter
// with half and quarter in {-1, 0, 1}; -3 = (-1, -1), -2 = (-1, 0), -1 = (0, -1), 0, 1 = (0, 1),
// 2 = (1, 0), 3 = (1, 1).  (Not the split xPatternSearchFracDIF would reach the position by.)
FME_DIRECT_HD int direct_half(int o) { return o <= -2 ? -1 : o >= 2 ? 1 : 0; }
FME_DIRECT_HD int direct_qtr(int o) { return o - 2 * direct_half(o); }

// The position as xPredInterBlk splits a quarter-pel MV component: integer part o >> 2 (-1 for a
// negative offset), fraction o & 3.  Class 24 is the integer position (0, 0 / 0, 0).
FME_DIRECT_HD int direct_int(int o) { return o < 0 ? -1 : 0; }
FME_DIRECT_HD int direct_frac(int o) { return o < 0 ? o + 4 : o; }

// half_x, half_y, qtr_x, qtr_y of a class as fme_result packs them (one byte each, in that order).
FME_DIRECT_HD uint32_t direct_half_qtr_word(int cls) {
  const int ox = direct_dx(cls), oy = direct_dy(cls);
  return (uint32_t)(uint8_t)direct_half(ox) | ((uint32_t)(uint8_t)direct_half(oy) << 8) |
         ((uint32_t)(uint8_t)direct_qtr(ox) << 16) | ((uint32_t)(uint8_t)direct_qtr(oy) << 24);
}

// The entry points' argument check: 0 (run), 1 (n == 0: nothing to do) or a negative FME_E_* code.
// out: the result array of the call's form.
inline int direct_request(const void* ctx, const void* jobs, const void* out, int n, int nn_mode) {
  if (!ctx || n < 0 || (n > 0 && (!jobs || !out))) return FME_E_INVALID;
  if (nn_mode == 0) return FME_E_STATE;   // no class to evaluate
  return n == 0 ? 1 : 0;
}

}  // namespace fme
