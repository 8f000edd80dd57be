// fme_direct_eval.h — the one sub-pel evaluation per job that an NN-direct batch (fme_direct.hip) and
// an external-predictor batch (fme_extern.hip) share, as the kernel template k_direct_eval<k10, Args>,
// with the per-job state both files' kernels keep in LDS.  The lanes, the prediction, the distortion
// and the tail are described in fme_direct.hip; k_direct_eval<k10, DirectArgs> is the kernel as it
// stood there.  With ExternArgs (kExt) it does what include/fme_extern.h asks for: the class comes
// from the caller's array, a job can be refused on its own, and the record's EMI fields can come
// from a row of NN inputs.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "fme_device.h"
#include "fme_direct_host.h"
#include "fme_extern_host.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"
#include "fme_unit_target.h"
#include "fme_xlane.h"

namespace fme {
namespace di {

using namespace simd;
using namespace mcl;
using namespace xlane;

constexpr int kDiBlock = 256;
constexpr int kDiTasks = kGroupTasks;   // consecutive jobs per workgroup, set up by its first wave

typedef uint32_t di_u4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t di_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef __attribute__((address_space(1))) di_u4 g_di_u4;
typedef __attribute__((address_space(1))) di_u2 g_di_u2;
typedef __attribute__((address_space(1))) uint32_t g_di_u32;
typedef __attribute__((address_space(1))) const di_u4 g_di_cu4;

// Per-job state shared by the workgroup (LDS), filled by one thread per job.
struct DiInfo {
  const uint8_t* ref;
  const uint8_t* org;
  const int16_t* key;         // the job's key block (rows of w), or null: the original at (x, y)
  int rstride, ral;           // reference stride, dword-aligned rows
  int ostride, oal;
  int pw, ph;                 // the reference picture's size
  int x, y, w, uxn, units;    // units 0: the job has no work in this kernel
  int lanes, start;           // lane group size (0: no work) and first lane slot
  int mode;                   // EMI: bit 0 the SAD metric, bit 1 FEN row subsampling; evaluation: kDist*
  int bx, by;                 // added to a unit's origin: the integer MV (evaluation: + the offset's integer part)
  int fx, fy;                 // evaluation: the quarter-pel fractions
};

// What both kernels' first wave does per job: the pictures, the target and the unit counts.
__device__ __forceinline__ void di_fill(const BatchArgs& a, const fme_job& j, DiInfo& in) {
  const PicDesc p = a.pics[j.ref_id];
  in.ref = p.luma;
  in.rstride = p.stride;
  in.ral = dword_rows(p.luma, p.stride);
  in.pw = p.width;
  in.ph = p.height;
  in.key = nullptr;
  in.org = nullptr;
  in.ostride = 0;
  in.oal = 0;
  if (j.key_offset >= 0) {
    in.key = a.keys + j.key_offset;
  } else {
    const PicDesc o = a.pics[j.org_id];
    in.org = o.luma;
    in.ostride = o.stride;
    in.oal = dword_rows(o.luma, o.stride) && (j.x & 3) == 0;
  }
  in.x = j.x;
  in.y = j.y;
  in.w = j.w;
  in.uxn = j.w >> 2;
  in.units = (j.w >> 2) * (j.h >> 2);
}

// One 16-byte row of a record or an NN input row.
__device__ __forceinline__ di_u4 di_ld16(const void* p, int k) { return ((g_di_cu4*)p)[k]; }

// The kernel of both files: Args is DirectArgs (k_direct_eval as it stood in fme_direct.hip) or
// ExternArgs (kExt).
__device__ __forceinline__ const DirectArgs& eval_direct(const DirectArgs& d) { return d; }
__device__ __forceinline__ const DirectArgs& eval_direct(const ExternArgs& x) { return x.d; }
__device__ __forceinline__ AtArgs eval_at(const DirectArgs&) { return AtArgs{}; }
__device__ __forceinline__ AtArgs eval_at(const ExternArgs& x) { return x.at; }

template <bool k10, class Args>
__global__ __launch_bounds__(kDiBlock) void k_direct_eval(Args args) {
  constexpr bool kExt = !std::is_same<Args, DirectArgs>::value;
  const DirectArgs& d = eval_direct(args);
  [[maybe_unused]] const AtArgs at = eval_at(args);
  const BatchArgs& a = d.a;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kDiTasks;
  const int nt = min(kDiTasks, d.n - t0);   // jobs of this workgroup (> 0 by the grid)
  if (d.sched->invalid) {   // a rejected batch: the tail marked the full records; the compact ones here
    if constexpr (kExt) {   // (no tail ran: every record is marked here, and 0 otherwise)
      if (t < nt) {
        const di_u4 z{0u, 0u, 0u, 0u}, st{0u, 0u, 0u, (uint32_t)FME_RES_REJECTED << 16};
        if (d.mv_out) {
          *(g_di_u4*)(d.mv_out + t0 + t) = st;
        } else {
          g_di_u4* r = (g_di_u4*)(a.res + t0 + t);
          r[0] = z; r[1] = z; r[2] = z; r[3] = st;
        }
      }
    } else {
      if (d.mv_out && t < nt) d.mv_out[t0 + t].status = FME_RES_REJECTED;
    }
    return;
  }
  __shared__ DiInfo info[kDiTasks];
  __shared__ uint32_t dist[kDiTasks];
  __shared__ uint8_t slot_task[kGroupSlots];
  __shared__ int total_lanes;
  fme_job j{};   // first wave: lane t keeps job t0 + t, its integer MV, class and the record's last word
  int mvx = 0, mvy = 0, cls = 24;
  uint32_t last = 0;
  bool refused = false;   // kExt: this job alone
  fme_result from_row{};  // kExt with rows: the record's EMI fields
  if (t < kDiTasks) {
    DiInfo& in = info[t];
    int lanes = 0;
    dist[t] = 0u;
    in.units = 0;
    in.uxn = 1;
    in.mode = kDistSad;
    if (t < nt) {
      j = load_job(a, t0 + t);
      if constexpr (kExt) {
        cls = (int)at.cls[t0 + t];
        refused = !extern_class_ok(cls);
        if (at.rows) {
          const di_u4 q0 = di_ld16(at.rows + t0 + t, 0), q1 = di_ld16(at.rows + t0 + t, 1);
          const di_u4 q2 = di_ld16(at.rows + t0 + t, 2), q3 = di_ld16(at.rows + t0 + t, 3);
          const uint32_t qw[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                   q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
          fme_nn_row row;
          __builtin_memcpy(&row, qw, sizeof(row));
          refused = refused || !extern_row_ok(row, j.mv_x, j.mv_y);
          extern_row_record(row, from_row);
          mvx = from_row.mv_int_x;
          mvy = from_row.mv_int_y;
          last = from_row.n_emi;
        } else {
          const g_di_u32* rec = (const g_di_u32*)(a.res + t0 + t);
          const uint32_t mvw = rec[0];
          last = rec[15] & 0xFFu;   // n_emi
          mvx = (int16_t)(mvw & 0xFFFFu);
          mvy = (int16_t)(mvw >> 16);
        }
        if (refused) cls = 24;
      } else {
        const g_di_u32* rec = (const g_di_u32*)(a.res + t0 + t);
        const uint32_t mvw = rec[0];
        last = rec[15];   // n_emi, nn_class, status
        mvx = (int16_t)(mvw & 0xFFFFu);
        mvy = (int16_t)(mvw >> 16);
        cls = min((int)((last >> 8) & 0xFFu), kDirectClasses - 1);   // (a class always: nn_mode 0 is refused)
      }
      if (!kExt || !refused) {
        di_fill(a, j, in);
        const int ox = direct_dx(cls), oy = direct_dy(cls);
        in.bx = mvx + direct_int(ox);
        in.by = mvy + direct_int(oy);
        in.fx = direct_frac(ox);
        in.fy = direct_frac(oy);
        in.mode = dist_mode(a.use_hadamard && !(j.flags & FME_JOB_LOSSLESS), j.w, j.h);
        lanes = group_lanes(in.units);
      }
    }
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
    if constexpr (kExt) {   // the first wave, all of it: one count per workgroup
      const unsigned long long m = __ballot(refused);
      if (lane == 0 && m) atomicAdd(at.refused, (int)__popcll(m));
    }
  }
  __syncthreads();
  const int total = total_lanes;
  for (int g0 = 0; g0 < total; g0 += kDiBlock) {   // workgroup-uniform
    const int g = g0 + t;
    const bool act = g < total;
    const int q = act ? (int)slot_task[g >> 2] : 0;
    const DiInfo& in = info[q];
    const int G = act ? in.lanes : 64;
    const int li = g - in.start;
    const int units = act ? in.units : 0;
    for (int u = li; __any(u < units); u += G) {   // wave-uniform
      const bool valid = u < units;
      const int mode = in.mode, uxn = max(in.uxn, 1);
      int ux, uy;
      unit_xy(u, uxn, mode == kDistHad8, ux, uy);
      const int x = in.x + 4 * ux, y = in.y + 4 * uy;
      int p[4][4], o[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) p[r][c] = 0;
      if (valid) luma_pred<k10>(Plane{in.ref, in.rstride, in.pw, in.ph}, in.ral != 0, x + in.bx, y + in.by, in.fx, in.fy, true, p);
      unit_target<k10>(in, x, y, valid, o);
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) o[r][c] -= p[r][c];
      // the lanes of a quad share a job and a round: the cross-lane stages of an 8x8 tile see all four
      uint32_t acc = unit_dist(o, mode, lane, (u & 3) == 0);
      if (!valid) acc = 0;
      acc = group_sum(acc, G, lane);   // wave-uniform control flow: every lane of the wave is here
      if (valid && li == 0) dist[q] += acc;
    }
  }
  __syncthreads();
  if (t >= nt) return;
  // ---- the position's cost, the tail, the record ----
  const int i = t0 + t;
  if constexpr (kExt) {
    if (refused) {   // this job alone: 0 but for the status
      const di_u4 z{0u, 0u, 0u, 0u}, st{0u, 0u, 0u, (uint32_t)FME_RES_REJECTED << 16};
      if (d.mv_out) {
        *(g_di_u4*)(d.mv_out + i) = st;
      } else {
        g_di_u4* r = (g_di_u4*)(a.res + i);
        r[0] = z; r[1] = z; r[2] = z; r[3] = st;
      }
      return;
    }
  }
  const double ml = a.mlambda[j.lambda_id];
  const int fx = 4 * mvx + direct_dx(cls), fy = 4 * mvy + direct_dy(cls);
  const uint32_t dsum = dist[t] >> (k10 ? d.bit_depth - 8 : 0);
  const uint32_t frac_cost = dsum + mv_cost(ml, mv_bits(fx, fy, 0, j.mvp_x, j.mvp_y));
  uint32_t bits;
  const uint32_t cost = me_tail(j, ml, frac_cost, fx, fy, bits);
  const uint32_t status = kExt ? (uint32_t)(FME_RES_NN_DIRECT | FME_RES_NN_EXTERN) : ((last >> 16) | FME_RES_NN_DIRECT);
  const uint32_t mvw = (uint32_t)(uint16_t)fx | ((uint32_t)(uint16_t)fy << 16);
  if (d.mv_out) {
    *(g_di_u4*)(d.mv_out + i) = di_u4{mvw, cost, bits, (uint32_t)cls | (status << 16)};
  } else {
    uint8_t* r = reinterpret_cast<uint8_t*>(a.res + i);
    const di_u4 r0{(uint32_t)(uint16_t)mvx | ((uint32_t)(uint16_t)mvy << 16), mvw, direct_half_qtr_word(cls), frac_cost};
    if constexpr (kExt) {
      const uint32_t w15 = (last & 0xFFu) | ((uint32_t)cls << 8) | (status << 16);
      if (at.rows) {   // the whole record: the EMI fields are the row's
        g_di_u4* o = (g_di_u4*)r;
        o[0] = r0;
        o[1] = di_u4{cost, bits, from_row.c, from_row.emi[0]};
        o[2] = di_u4{from_row.emi[1], from_row.emi[2], from_row.emi[3], from_row.emi[4]};
        o[3] = di_u4{from_row.emi[5], from_row.emi[6], from_row.emi[7], w15};
      } else {
        *(g_di_u4*)r = r0;
        *(g_di_u2*)(r + 16) = di_u2{cost, bits};
        *(g_di_u32*)(r + 60) = w15;
      }
    } else {
      *(g_di_u4*)r = r0;
      *(g_di_u2*)(r + 16) = di_u2{cost, bits};
      *(g_di_u32*)(r + 60) = (last & 0xFFFFu) | (status << 16);
    }
  }
}

}  // namespace di
}  // namespace fme
