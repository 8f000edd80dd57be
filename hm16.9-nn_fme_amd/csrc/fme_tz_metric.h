// fme_tz_metric.h — the integer-ME metric of one unit (the NN_FME setDistParam, TComRdCost.cpp:200-230)
// at both bit depths: what the integer search (fme_tz.hip) prices its candidates with, its final
// square included, and what the NN-direct path's EMI kernel (fme_direct.hip) prices the same square
// with.  SSE for widths 4..64, SAD for 12/24/48 with the FEN even-row subsampling; the callers load
// the window and the key rows and sum the units of a PU.
#pragma once

#include <hip/hip_runtime.h>

#include "fme_simd.h"

namespace fme {
namespace tzm {

using namespace simd;

// One unit's share of the distortion (TComRdCost metric of the integer search) for a window.
// w: UH rows of UW / 4 + 1 dwords from the aligned column, s0 the byte shift of the first sample; kk: the
// key rows, org bytes (KW = UW / 4, or the first UW / 4 dwords of UW / 2) or int16 key pairs (kbuf, KW =
// UW / 2); sk2: the sum of the squared (s - 128) org bytes; sub: FEN, the even rows only, doubled.
template <int UW, int UH, int KW>
__device__ __forceinline__ uint32_t unit_part(const uint32_t (&w)[UH][UW / 4 + 1], uint32_t s0,
                                              const uint32_t (&kk)[UH][KW], int sk2, bool kbuf,
                                              bool sad_metric, bool sub) {
  int sop = 0, spp = 0;
  uint32_t acc = 0;
#pragma unroll
  for (int r = 0; r < UH; r++) {
    if (sub && (r & 1)) continue;
#pragma unroll
    for (int c = 0; c < UW / 4; c++) {
      const uint32_t pv = __builtin_amdgcn_alignbyte(w[r][c + 1], w[r][c], s0);   // reference bytes
      if (!kbuf) {
        if (sad_metric) {
          acc = __builtin_amdgcn_sad_u8(pv, kk[r][c], acc);
        } else {
          const uint32_t ps = pv ^ 0x80808080u;
          sop = dot4(kk[r][c] ^ 0x80808080u, ps, sop);
          spp = dot4(ps, ps, spp);
        }
      } else if constexpr (KW == UW / 2) {
        const uint32_t d0 = pk_sub(kk[r][2 * c], lo_pair(pv));
        const uint32_t d1 = pk_sub(kk[r][2 * c + 1], hi_pair(pv));
        if (sad_metric) {
          acc = udot2(pk_abs(d0), 0x00010001u, udot2(pk_abs(d1), 0x00010001u, acc));
        } else {
          acc = (uint32_t)dot2(d1, d1, dot2(d0, d0, (int)acc));
        }
      }
    }
  }
  uint32_t part = (!kbuf && !sad_metric) ? (uint32_t)(sk2 - 2 * sop + spp) : acc;
  if (sub) part <<= 1;
  return part;
}

// One unit's share of the bit-depth-10 distortion: SSE sums (d * d) >> 4 per sample
// (xGetSSE, TComRdCost.cpp:875-1130, DISTORTION_PRECISION_ADJUSTMENT(2 (bitDepth - 8))) as
// (sum d^2 - sum (d^2 mod 16)) >> 4, with d^2 mod 16 = ((d & 7)^2) & 15; SAD returns the raw sum
// (<< 1 with FEN subsampling), the block's >> 2 (xGetSAD12/24/48: uiSum >> (bitDepth - 8)) comes
// after the group sum.  kk: the key as sample pairs (org samples, or the bi-pred int16 key).
template <int UW, int UH>
__device__ __forceinline__ uint32_t unit_part10(const uint32_t (&w)[UH][UW / 2 + 1], uint32_t s0,
                                                const uint32_t (&kk)[UH][UW / 2], bool sad_metric, bool sub) {
  int sq = 0;
  uint32_t lo = 0, acc = 0;
#pragma unroll
  for (int r = 0; r < UH; r++) {
    if (sub && (r & 1)) continue;
#pragma unroll
    for (int c = 0; c < UW / 2; c++) {
      const uint32_t pv = s0 ? __builtin_amdgcn_alignbyte(w[r][c + 1], w[r][c], 2u) : w[r][c];
      const uint32_t dd = pk_sub(kk[r][c], pv);
      if (sad_metric) {
        acc = udot2(pk_abs(dd), 0x00010001u, acc);
      } else {
        sq = dot2(dd, dd, sq);
        // d^2 mod 16 by d & 7 (0 1 4 9 0 9 4 1) from a byte table: one v_and_or makes the v_perm
        // selector (byte 0x0C selects zero), the perm gives the pair of residues as u16 halves
        const uint32_t sel = (dd & 0x00070007u) | 0x0C000C00u;
        lo = udot2(__builtin_amdgcn_perm(0x01040900u, 0x09040100u, sel), 0x00010001u, lo);
      }
    }
  }
  if (sad_metric) return sub ? acc << 1 : acc;
  return ((uint32_t)sq - lo) >> 4;
}

}  // namespace tzm
}  // namespace fme
