// fme_mc_luma.h — xPredInterBlk's building blocks shared by the prediction kernels: motion
// compensation and the producers' luma stages (fme_mc.hip), the prediction error (fme_merge.hip), the
// skip check (fme_skip.hip) and the cost surface (fme_surface.hip: taps and window only).  The luma
// interpolation taps, clipMv, the edge-replicated reference window of one output unit and its
// two-stage filter at 8 and 10 bits behind one depth-dispatching predictor (unit_pred), the
// resolution of a PU's motion into its predicted lists (resolve_lists, ListMotion), the prediction
// of a unit from up to two lists (pred_lists, add_avg) and the checks the validity predicates share.
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
// bitDepth 10 shifts by 14 + 1 - 10 after adding 16 + 2 * 8192 (add_avg).
typedef __attribute__((address_space(1))) const uint16_t gu16c;

// pl.p points at uint16 samples, pl.stride counts samples.
template <int N, int U>
__device__ __forceinline__ void pred10(const Plane& pl, int bx, int by, uint32_t hlo, uint32_t hhi, uint32_t vlo,
                                       uint32_t vhi, bool uni, int (&out)[U][U]) {
  constexpr int R = U + N - 1;
  const int x0 = bx - (N / 2 - 1), y0 = by - (N / 2 - 1);
  const uint16_t* px = reinterpret_cast<const uint16_t*>(pl.p);
  int h[R][U];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const gu16c* row = (const gu16c*)(px + (size_t)clamp_i(y0 + r, 0, pl.h - 1) * pl.stride);
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

// Sample i of a plane at either depth (k10: plane holds uint16 samples).
template <bool k10>
__device__ __forceinline__ int ld_sample(const uint8_t* plane, size_t i) {
  if constexpr (k10) return (int)((const gu16c*)reinterpret_cast<const uint16_t*>(plane))[i];
  else return (int)gld8(plane + i);
}

// One U x U unit of one list at either depth (k10: uint16 planes, pred10; else UnitWin).
template <bool k10, int N, int U>
__device__ __forceinline__ void unit_pred(const Plane& pl, bool aligned, int bx, int by, uint32_t hlo, uint32_t hhi,
                                          uint32_t vlo, uint32_t vhi, bool uni, int (&out)[U][U]) {
  if constexpr (k10) {
    pred10<N, U>(pl, bx, by, hlo, hhi, vlo, vhi, uni, out);
  } else {
    UnitWin<N, U> w;
    w.load(pl, aligned, bx, by);
    w.pred(hlo, hhi, vlo, vhi, uni, out);
  }
}

// The 4x4 luma unit at plane position (bx, by) (integer MV applied), quarter-pel fractions (fx, fy).
template <bool k10>
__device__ __forceinline__ void luma_pred(const Plane& pl, bool aligned, int bx, int by, int fx, int fy, bool uni,
                                          int (&o)[4][4]) {
  uint32_t hlo, hhi, vlo, vhi;
  luma_taps(fx, hlo, hhi);
  luma_taps(fy, vlo, vhi);
  unit_pred<k10, 8, 4>(pl, aligned, bx, by, hlo, hhi, vlo, vhi, uni, o);
}
__device__ __forceinline__ Plane luma_plane(const PicDesc& p) { return Plane{p.luma, p.stride, p.width, p.height}; }
__device__ __forceinline__ bool dword_rows(const uint8_t* p, int stride) { return ((stride | (int)(uintptr_t)p) & 3) == 0; }

// One predicted list of a PU's motion: its picture and the clipped MV split as xPredInterBlk does
// (shift 2 + csx, fraction mask (4 << csx) - 1) for luma and 4:2:0 chroma.
struct ListMotion {
  PicDesc pic;
  int lix, liy, lfx, lfy;   // luma integer offset, quarter-pel fraction
  int cix, ciy, cfx, cfy;   // chroma integer offset, eighth-pel fraction (unused by luma-only callers)
};

// The lists a PU's motion predicts from (flags: FME_MC_L0 | FME_MC_L1), in list order, into lm[0 .. nl):
// clipMv against the CU origin and, where the caller lets it apply, xCheckIdenticalMotion
// (TComPrediction.cpp:476-492): both lists on one picture with one MV -> xPredInterUni(REF_PIC_LIST_0).
// Selects, not reads indexed by the list: the job stays in registers.
__device__ __forceinline__ int resolve_lists(uint32_t flags, const uint8_t (&ref_id)[2], const int16_t (&mv)[2][2],
                                             int cu_x, int cu_y, const PicDesc* pics, bool check_identical,
                                             ListMotion (&lm)[2]) {
  const int r0 = ref_id[0], r1 = ref_id[1], x0 = mv[0][0], y0 = mv[0][1], x1 = mv[1][0], y1 = mv[1][1];
  int nl = ((flags & FME_MC_L0) ? 1 : 0) + ((flags & FME_MC_L1) ? 1 : 0);
  if (check_identical && nl == 2 && r0 == r1 && x0 == x1 && y0 == y1) nl = 1;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (k >= nl) break;
    const bool l1 = k == 1 || !(flags & FME_MC_L0);   // the k-th predicted list is list 1
    ListMotion& m = lm[k];
    m.pic = pics[l1 ? r1 : r0];
    int mx = l1 ? x1 : x0, my = l1 ? y1 : y0;
    clip_mv(mx, my, m.pic.width, m.pic.height, cu_x, cu_y);
    m.lix = mx >> 2;
    m.liy = my >> 2;
    m.lfx = mx & 3;
    m.lfy = my & 3;
    m.cix = mx >> 3;
    m.ciy = my >> 3;
    m.cfx = mx & 7;
    m.cfy = my & 7;
  }
  return nl;
}

// One list's prediction of the 4x4 luma unit at (x, y).
template <bool k10>
__device__ __forceinline__ void list_luma(const ListMotion& m, int x, int y, bool uni, int (&o)[4][4]) {
  luma_pred<k10>(luma_plane(m.pic), dword_rows(m.pic.luma, m.pic.stride), x + m.lix, y + m.liy, m.lfx, m.lfy, uni, o);
}

// TComYuv::addAvg of the two lists' 14-bit values (TComYuv.cpp:354-415): shift 15 - bitDepth, offset
// half of it + 2 * 8192, clipped to the bit depth.
template <bool k10>
__device__ __forceinline__ int add_avg(int p0, int p1) {
  return k10 ? clamp_i((p0 + p1 + 16400) >> 5, 0, 1023) : clamp_i((p0 + p1 + 16448) >> 7, 0, 255);
}

// A unit's prediction from its nl (1 or 2) lists.  one(k, o) predicts list k into o: clipped samples
// when it is the only list (uni), else 14-bit values.  p = the only list's samples or add_avg of the
// two; l0 and l1 keep the values of list 0 and of the last list predicted (weighted prediction
// combines those itself).
template <bool k10, class F, int U>
__device__ __forceinline__ void pred_lists(int nl, F one, int (&p)[U][U], int (&l0)[U][U], int (&l1)[U][U]) {
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (k >= nl) break;
    one(k, l1);
#pragma unroll
    for (int r = 0; r < U; r++)
#pragma unroll
      for (int c = 0; c < U; c++) {
        if (k == 0) l0[r][c] = l1[r][c];
        p[r][c] = k == 0 ? l1[r][c] : add_avg<k10>(p[r][c], l1[r][c]);
      }
  }
}
template <bool k10, class F, int U>
__device__ __forceinline__ void pred_lists(int nl, F one, int (&p)[U][U]) {
  int l0[U][U], l1[U][U];
  pred_lists<k10>(nl, one, p, l0, l1);
}

// What the validity predicates of the prediction kernels share: a PU is 4..64 samples in steps of 4,
// and every predicted list names a pw x ph picture that has luma (and chroma where asked).
__device__ __forceinline__ bool pu_shape_ok(int w, int h) {
  return w >= 4 && h >= 4 && w <= 64 && h <= 64 && !(w & 3) && !(h & 3);
}
__device__ __forceinline__ bool ref_ok(bool used, int id, const PicDesc* pics, int pw, int ph, bool chroma) {
  if (!used) return true;
  if (id >= FME_MAX_PICTURES) return false;
  const PicDesc& p = pics[id];
  return p.luma && (!chroma || (p.cb && p.cr)) && p.width == pw && p.height == ph;
}
// (no loop over the lists: a read indexed by the list would put the job into scratch)
__device__ __forceinline__ bool refs_ok(uint32_t flags, const uint8_t (&ref_id)[2], const PicDesc* pics, int pw, int ph,
                                        bool chroma) {
  return ref_ok(flags & FME_MC_L0, ref_id[0], pics, pw, ph, chroma) &&
         ref_ok(flags & FME_MC_L1, ref_id[1], pics, pw, ph, chroma);
}

}  // namespace mcl
}  // namespace fme
