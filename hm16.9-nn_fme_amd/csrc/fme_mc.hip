// fme_mc.hip — motion compensation of decided MVs (gfx950): luma 8-tap + 4:2:0 chroma 4-tap.
//
// TComPrediction::motionCompensation (TComPrediction.cpp:495-560): a few PUs per workgroup, one
// 4x4 luma unit (+ the co-sited 2x2 Cb and Cr units) per lane, reference windows in VGPRs:
//   * clipMv of each list's MV against the CU origin (TComDataCU.cpp:2773-2786);
//   * xCheckIdenticalMotion (TComPrediction.cpp:476-492): both lists on one picture with one MV
//     -> uni-prediction from L0;
//   * xPredInterBlk (616-668) per component: integer offset mv >> (2 + csx), fraction
//     mv & ((4 << csx) - 1); HM copies at fraction (0,0), filters once at (fx,0) / (0,fy) and
//     twice otherwise (TComInterpolationFilter.cpp:94-154 filterCopy, 172-257 filter<N, isVert,
//     isFirst, isLast>).  Here every case runs the two-stage form with the identity filter
//     (64 at the centre tap) for a zero fraction, which gives the same integers: with
//     S = sum c.s and s' = s - 128 (sum c = 64), stage 1 = S - 8192 = sum c.s'; a zero vertical
//     fraction multiplies it by 64, and (64 (S - 8192) + 2048 + (8192 << 6)) >> 12 = (S + 32)
//     >> 6 (uni), (64 (S - 8192)) >> 6 = S - 8192 (bi); a zero horizontal fraction gives
//     stage 1 = 64 s' = (s << 6) - 8192, filterCopy's isFirst output.  Uni-prediction ends at
//     the bit depth, bi-prediction keeps the 14-bit values;
//   * TComYuv::addAvg (TComYuv.cpp:354-415) of the two lists' 14-bit values (add_avg).
// Samples outside a plane are read with edge replication, which equals HM's padded picture for
// every clipped MV (luma margin 80, chroma margin 40: the clipped reads stay within 75 / 38).
// Every kernel is one text for both bit depths (template <bool k10>: uint16 planes, strides in
// samples); the list resolution, the unit predictors and the two-list average are fme_mc_luma.h's
// and fme_mc_chroma.h's, shared with fme_merge.hip and fme_skip.hip.
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_mc_chroma.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"

namespace fme {
namespace {

using namespace simd;
using namespace mcl;

__device__ __forceinline__ bool mc_job_valid(const McArgs& a, const fme_mc_job& j) {
  if (!pu_shape_ok(j.w, j.h)) return false;
  if (!(j.flags & (FME_MC_L0 | FME_MC_L1)) || (j.flags & ~(FME_MC_L0 | FME_MC_L1 | FME_MC_WP))) return false;
  if ((int)j.x + j.w > a.width || (int)j.y + j.h > a.height) return false;
  return refs_ok(j.flags, j.ref_id, a.pics, a.width, a.height, true);
}

// n (4 or 2) samples of one output row at sample offset off of plane.  8 bits: one packed dword /
// word store, per byte when the plane's rows are not aligned to it; 10 bits: 16-bit stores.
template <bool k10>
__device__ __forceinline__ void store_row(uint8_t* plane, size_t off, const int* v, int n, bool aligned) {
  if constexpr (k10) {
    uint16_t* d = reinterpret_cast<uint16_t*>(plane) + off;
    for (int i = 0; i < n; i++) d[i] = (uint16_t)v[i];
  } else {
    uint8_t* d = plane + off;
    if (n == 4 && aligned) {
      *(uint32_t*)d = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else if (n == 2 && aligned) {
      *(uint16_t*)d = (uint16_t)((uint32_t)v[0] | ((uint32_t)v[1] << 8));
    } else {
      for (int i = 0; i < n; i++) d[i] = (uint8_t)v[i];
    }
  }
}

// Per-job state shared by the workgroup (LDS), filled by one thread per job.
struct McJobInfo {
  int units;          // 4x4 luma units, 0 when invalid
  int ux_n;           // units per PU row
  int x, y;           // PU luma origin
  int nl;             // lists predicted (2: bi)
  ListMotion lm[2];   // per predicted list
  int wp;                              // FME_MC_WP: weighted prediction of the lists' 14-bit values
  int ww[2][3], wsh[3], woff[3];       // per component: the lists' weights, shift, (summed) offset
};

// getWpScaling (TComWeightPrediction.cpp:247-324) for the PU's lists, per component: bi-pred
// w0 / w1, offset o0 + o1, shift log2Wd + 1 (list 0's denominator); uni-pred w, o, shift log2Wd;
// offsets scaled by 1 << (bitDepth - 8); addWeightBi / addWeightUni then add shiftNum =
// max(2, 14 - bitDepth) (:103, :160).
__device__ __forceinline__ void mc_wp_setup(const McArgs& a, const fme_mc_job& j, int nl, McJobInfo& in) {
  const int bd = a.bit_depth > 8 ? a.bit_depth : 8;
  const int shift_num = 14 - bd > 2 ? 14 - bd : 2;
  // the first predicted list's row of wp[list][picture]
  const int first = (j.flags & FME_MC_L0) ? j.ref_id[0] : FME_MAX_PICTURES + j.ref_id[1];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const fme_wp_param p0 = a.wp[first * 3 + c];
    in.ww[0][c] = p0.weight;
    if (nl == 2) {
      const fme_wp_param p1 = a.wp[(FME_MAX_PICTURES + j.ref_id[1]) * 3 + c];
      in.ww[1][c] = p1.weight;
      in.woff[c] = (p0.offset + p1.offset) * (1 << (bd - 8));
      in.wsh[c] = p0.log2_denom + 1 + shift_num;
    } else {
      in.ww[1][c] = 0;
      in.woff[c] = p0.offset * (1 << (bd - 8));
      in.wsh[c] = p0.log2_denom + shift_num;
    }
  }
}

// weightBidir / weightUnidir (TComWeightPrediction.cpp:46-56) on the 14-bit values p0, p1 (HM's
// stored intermediates, IF_INTERNAL_OFFS 8192 below the sample scale).  The unit-weight branch of
// addWeightUni (noWeightUnidir with shiftNum) is the same value: w = 1 << d turns
// (w (p + 8192) + 2^(d + n - 1)) >> (d + n) into (p + 8192 + 2^(n - 1)) >> n exactly.
__device__ __forceinline__ int mc_wp_sample(const McJobInfo& in, int c, int p0, int p1, int maxv) {
  const int sh = in.wsh[c], half = 1 << (sh - 1);
  if (in.nl == 2)
    return clamp_i((in.ww[0][c] * (p0 + 8192) + in.ww[1][c] * (p1 + 8192) + half + in.woff[c] * half) >> sh, 0, maxv);
  return clamp_i(((in.ww[0][c] * (p0 + 8192) + half) >> sh) + in.woff[c], 0, maxv);
}

#ifndef FME_MC_JOBS
#define FME_MC_JOBS 8
#endif
constexpr int kMcJobs = FME_MC_JOBS;   // consecutive jobs per workgroup
constexpr int kMcBlock = 256;

// The U x U unit of component comp at (x, y) of its plane: one(k, o) predicts list k; the lists
// are averaged, or weighted from their 14-bit values, and stored.
template <bool k10, int U, class F>
__device__ __forceinline__ void mc_unit(const McJobInfo& in, int comp, F one, uint8_t* plane, int stride, int x, int y,
                                        bool aligned) {
  int acc[U][U], q0[U][U], o[U][U];
  pred_lists<k10>(in.nl, one, acc, q0, o);
  if (in.wp)
#pragma unroll
    for (int r = 0; r < U; r++)
#pragma unroll
      for (int c = 0; c < U; c++) acc[r][c] = mc_wp_sample(in, comp, q0[r][c], o[r][c], k10 ? 1023 : 255);
#pragma unroll
  for (int r = 0; r < U; r++) store_row<k10>(plane, (size_t)(y + r) * stride + x, acc[r], U, aligned);
}

// kMcJobs consecutive jobs per workgroup; their 4x4 luma units (each with the co-sited 2x2 Cb and
// Cr units) are dealt to the 256 lanes, so small and large PUs fill the waves alike; a lane
// predicts both lists of its unit in registers and averages them.
template <bool k10>
__global__ __launch_bounds__(kMcBlock) void k_mc(McArgs a) {
  __shared__ McJobInfo info[kMcJobs];
  __shared__ int first_unit[kMcJobs + 1];
  const int j0 = blockIdx.x * kMcJobs;
  const int t = threadIdx.x;
  if (t < kMcJobs) {
    McJobInfo& in = info[t];
    in.units = 0;
    const int ji = j0 + t;
    if (ji < a.n) {
      const fme_mc_job j = a.jobs[ji];
      if (!mc_job_valid(a, j)) {
        atomicAdd(a.invalid, 1);
      } else {
        const bool wp = (j.flags & FME_MC_WP) != 0;
        // xCheckIdenticalMotion does not apply with WPBiPred
        const int nl = resolve_lists(j.flags, j.ref_id, j.mv, j.cu_x, j.cu_y, a.pics, !wp, in.lm);
        in.wp = wp ? 1 : 0;
        in.nl = nl;
        if (wp) mc_wp_setup(a, j, nl, in);
        in.x = j.x;
        in.y = j.y;
        in.ux_n = j.w >> 2;
        in.units = (j.w >> 2) * (j.h >> 2);
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < kMcJobs; k++) {
      first_unit[k] = acc;
      acc += info[k].units;
    }
    first_unit[kMcJobs] = acc;
  }
  __syncthreads();
  const int total = first_unit[kMcJobs];
  const bool ys_al = ((a.y_stride | (int)(uintptr_t)a.y) & 3) == 0;
  const bool cs_al = ((a.c_stride | (int)(uintptr_t)a.cb | (int)(uintptr_t)a.cr) & 1) == 0;
  for (int g = t; g < total; g += kMcBlock) {
    int q = 0;
#pragma unroll
    for (int k = 1; k < kMcJobs; k++) q += g >= first_unit[k] ? 1 : 0;
    const McJobInfo& in = info[q];
    const int u = g - first_unit[q];
    const int ux = u % in.ux_n, uy = u / in.ux_n;
    const bool uni = in.nl == 1 && !in.wp;   // weighted prediction filters to the 14-bit values (bi form)
    {   // luma 4x4
      const int x = in.x + 4 * ux, y = in.y + 4 * uy;
      mc_unit<k10, 4>(in, 0, [&](int k, int (&o)[4][4]) { list_luma<k10>(in.lm[k], x, y, uni, o); }, a.y, a.y_stride, x,
                      y, ys_al);
    }
#pragma unroll
    for (int comp = 1; comp <= 2; comp++) {   // chroma 2x2 of Cb and Cr (4:2:0)
      const int x = (in.x >> 1) + 2 * ux, y = (in.y >> 1) + 2 * uy;
      mc_unit<k10, 2>(in, comp, [&](int k, int (&o)[2][2]) { list_chroma<k10>(in.lm[k], comp, x, y, uni, o); },
                      comp == 1 ? a.cb : a.cr, a.c_stride, x, y, cs_al);
    }
  }
}

// One task per wave (AmvpTask, BiKeyTask): clipMv of the task's MV against the CU origin and the
// uni-pred luma prediction xPredInterBlk(COMPONENT_Y, ..., bi = false) of its PU from ref; the
// lanes walk the PU's 4x4 units and hand each unit's samples to unit(ux, uy, o).
template <bool k10, class Task, class F>
__device__ __forceinline__ void wave_luma_units(const Task& t, const PicDesc& ref, int lane, F unit) {
  int mx = t.mv_x, my = t.mv_y;
  clip_mv(mx, my, ref.width, ref.height, t.cu_x, t.cu_y);
  const bool al = dword_rows(ref.luma, ref.stride);
  const int uxn = t.w >> 2, units = uxn * (t.h >> 2);
  for (int u = lane; u < units; u += 64) {
    const int ux = u % uxn, uy = u / uxn;
    int o[4][4];
    luma_pred<k10>(luma_plane(ref), al, t.x + 4 * ux + (mx >> 2), t.y + 4 * uy + (my >> 2), mx & 3, my & 3, true, o);
    unit(ux, uy, o);
  }
}

// xGetTemplateCost (TEncSearch.cpp:4397-4436) distortion: the prediction at the candidate and
// getDistPart(DF_SAD) against the original (plain SAD at every width: setDistParam(UInt, UInt,
// DFunc) sets no subsampling, TComRdCost.cpp:187-197).  At bitDepth 10 xGetSAD* shifts the block
// sum >> 2 (uiSum >> DISTORTION_PRECISION_ADJUSTMENT(bitDepth - 8), TComRdCost.cpp:370-536).
template <bool k10>
__global__ __launch_bounds__(kMcBlock) void k_amvp_sad(AmvpArgs a) {
  const int task = (int)(blockIdx.x * (kMcBlock / 64) + (threadIdx.x >> 6));
  if (task >= a.n) return;   // wave-uniform
  const int lane = (int)(threadIdx.x & 63);
  const AmvpTask t = a.tasks[task];
  const PicDesc ref = a.pics[t.ref_id], org = a.pics[t.org_id];
  uint32_t sad = 0;
  wave_luma_units<k10>(t, ref, lane, [&](int ux, int uy, const int (&o)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const size_t row = (size_t)(t.y + 4 * uy + r) * org.stride + t.x + 4 * ux;
#pragma unroll
      for (int c = 0; c < 4; c++) sad += (uint32_t)abs(o[r][c] - ld_sample<k10>(org.luma, row + c));
    }
  });
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sad += (uint32_t)__shfl_xor((int)sad, off, 64);
  if (lane == 0) a.sad[task] = k10 ? sad >> 2 : sad;
}

// Device-resident requests (fme_build_bipred_keys_device, a.invalid set): the host checks' equivalent;
// a rejected request is counted once (lane 0) and skipped.
__device__ __forceinline__ bool bi_key_task_ok(const BiKeyArgs& a, const BiKeyTask& t, int lane) {
  if (!a.invalid) return true;
  bool shape = false;
#pragma unroll
  for (int k = 0; k < kNumClasses; k++) shape |= kClassW[k] == t.w && kClassH[k] == t.h;
  bool ok = shape && t.org_id < FME_MAX_PICTURES && t.ref_id < FME_MAX_PICTURES && t.key_off >= 0 &&
            (t.key_off & 3) == 0 && (int64_t)t.key_off + (int64_t)t.w * t.h <= a.n_keys &&
            (t.clip & ~FME_PU_CLIP_BIPRED) == 0;
  if (ok) {
    const PicDesc r = a.pics[t.ref_id], o = a.pics[t.org_id];
    ok = r.luma && o.luma && r.width == o.width && r.height == o.height && t.x + t.w <= o.width &&
         t.y + t.h <= o.height;
  }
  if (!ok && lane == 0) atomicAdd(a.invalid, 1);
  return ok;
}

// xMotionEstimation(bBi) (TEncSearch.cpp:4461-4471): motionCompensation of the other list (luma,
// uni-pred) and TComYuv::removeHighFreq (TComYuv.cpp:411-455) into the key buffer: 2 * org - pred,
// with ClipForBiPredMe ClipBD to the bit depth.
template <bool k10>
__global__ __launch_bounds__(kMcBlock) void k_bi_key(BiKeyArgs a) {
  const int task = (int)(blockIdx.x * (kMcBlock / 64) + (threadIdx.x >> 6));
  if (task >= a.n) return;   // wave-uniform
  const int lane = (int)(threadIdx.x & 63);
  const BiKeyTask t = a.tasks[task];
  if (!bi_key_task_ok(a, t, lane)) return;   // wave-uniform
  const PicDesc ref = a.pics[t.ref_id], org = a.pics[t.org_id];
  wave_luma_units<k10>(t, ref, lane, [&](int ux, int uy, const int (&o)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const size_t row = (size_t)(t.y + 4 * uy + r) * org.stride + t.x + 4 * ux;
      int16_t* kp = a.keys + t.key_off + (size_t)(4 * uy + r) * t.w + 4 * ux;
      int v[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        v[c] = 2 * ld_sample<k10>(org.luma, row + c) - o[r][c];
        if (t.clip) v[c] = clamp_i(v[c], 0, k10 ? 1023 : 255);
      }
      // 4 int16 = 8 bytes; key_off and w are multiples of 4, so the store is 8-byte aligned
      *(uint2*)kp = make_uint2((uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16),
                               (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16));
    }
  });
}

}  // namespace

hipError_t launch_bi_key(const BiKeyArgs& a, hipStream_t s) {
  return launch_by_depth(k_bi_key<false>, k_bi_key<true>, (a.n + kMcBlock / 64 - 1) / (kMcBlock / 64), kMcBlock, a, s);
}

hipError_t launch_mc(const McArgs& a, hipStream_t s) {
  return launch_by_depth(k_mc<false>, k_mc<true>, (a.n + kMcJobs - 1) / kMcJobs, kMcBlock, a, s);
}

hipError_t launch_amvp_sad(const AmvpArgs& a, hipStream_t s) {
  return launch_by_depth(k_amvp_sad<false>, k_amvp_sad<true>, (a.n + kMcBlock / 64 - 1) / (kMcBlock / 64), kMcBlock, a, s);
}

}  // namespace fme
