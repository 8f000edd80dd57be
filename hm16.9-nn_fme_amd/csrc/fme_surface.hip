// fme_surface.hip — the sub-pel cost surface of a PU on the GPU (gfx950): the distortion and cost of
// all 49 quarter-pel positions within +-3/4 pel of the job's integer MV (include/fme_surface.h).
//
// Per job and offset (dx, dy), each in -3..3: the normative luma prediction at the quarter-pel MV
// (4 mv_x + dx, 4 mv_y + dy) (xPredInterBlk: two-stage 8-tap filter, 14-bit intermediates, uni-pred,
// clipped; no clipMv, picture edges replicated), FracDIF's distortion against the original or the
// job's key block (TComRdCost.cpp:233-275: xGetHADs with 8x8 or 4x4 tiles, or the SAD; the PU's sum
// >> bitDepth - 8 once) and cost = dist + (UInt)(mlambda * bits / 65536.0) with the quarter-pel bits
// of the MV difference to mvp.
//
// Lanes: k_pred_err's (fme_merge.hip).  One lane per 4x4 unit; a job's lane group is its unit count
// rounded up to a power of two between 4 and 64 (a PU of more than 64 units walks them in steps of
// 64); a workgroup takes 64 consecutive jobs and packs their groups largest class first; with 8x8
// Hadamards the four quadrants of a tile sit in four consecutive lanes and two DPP butterfly stages
// join their 4x4 transforms.
//
// The filter stages are shared between positions.  An offset dx < 0 has integer part -1 and fraction
// dx + 4, an offset dx >= 0 integer part 0 and fraction dx, so the 49 positions read the 12x12
// samples at rows and columns -4..+7 around the unit's origin at the integer MV.  The lane loads that
// window once; per dx it filters the twelve rows horizontally once (12x4 intermediates, the column
// offset 0 or 1 a template parameter so that every register index is static) and reuses them for
// the seven dy: 7 first stages per unit instead of 49.  The identity filter at fraction 0 reproduces
// filterCopy and the 1-D filters exactly in the two-stage form (fme_mc_luma.h), so one code path
// serves all 49 positions.  Group sums go through the DPP / permlane steps; the group's first lane
// adds them to the job's row in LDS, where the costs, the pick and the 16-byte output rows are made
// once all units are in.
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_mc_luma.h"
#include "fme_simd.h"
#include "fme_surface_host.h"
#include "fme_unit_target.h"
#include "fme_xlane.h"

namespace fme {
namespace {

using namespace simd;
using namespace mcl;
using namespace xlane;

constexpr int kSfBlock = 256;
constexpr int kSfTasks = kGroupTasks;   // consecutive jobs per workgroup, set up by its first wave
constexpr int kSfWords = 2 * FME_SURF_POINTS;   // words of one fme_surface

typedef uint32_t sf_u4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t sf_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef __attribute__((address_space(1))) sf_u4 g_sf_u4;
typedef __attribute__((address_space(1))) sf_u2 g_sf_u2;

// Per-job state shared by the workgroup (LDS), filled by one thread per job.
struct SfInfo {
  const uint8_t* ref;
  const uint8_t* org;
  const int16_t* key;         // the job's key block (rows of w), or null: the original at (x, y)
  double ml;
  int rstride, ral;           // reference stride, dword-aligned rows
  int ostride, oal;
  int pw, ph;                 // the reference picture's size
  int x, y, w, uxn, units;
  int lanes, start;           // lane group size (0: no work) and first lane slot
  int mode, valid;
  int mvx, mvy, mvpx, mvpy;
  int probe0, probe1;
};

__device__ __forceinline__ bool sf_job_valid(const SurfArgs& a, const fme_job& j, unsigned p0, unsigned p1) {
  if (!surf_shape_ok(j.w, j.h) || !surf_probe_ok(p0) || !surf_probe_ok(p1)) return false;
  if (j.ref_id >= FME_MAX_PICTURES || j.lambda_id >= FME_MAX_LAMBDAS) return false;
  const PicDesc& r = a.pics[j.ref_id];
  if (!r.luma) return false;
  if (j.key_offset >= 0) return (int64_t)j.key_offset + (int64_t)j.w * j.h <= a.n_keys;
  if (j.org_id >= FME_MAX_PICTURES) return false;
  const PicDesc& o = a.pics[j.org_id];
  return o.luma && o.width == r.width && o.height == r.height && (int)j.x + j.w <= o.width && (int)j.y + j.h <= o.height;
}

// The unit's 12x12 window at rows and columns -4..+7 around plane position (bx, by), and the first
// filter stage at column offset OX (0: integer part -1, 1: integer part 0) and fraction fx.
template <bool k10>
struct SfWin;

template <>
struct SfWin<false> {
  uint32_t a[12][3];   // rows of (s - 128) bytes, re-aligned to the window's first column
  __device__ __forceinline__ void load(const SfInfo& in, int bx, int by, bool valid) {
    if (valid) {
      uint32_t w[12][4];
      const uint32_t s0 = load_window<12, 4>(Plane{in.ref, in.rstride, in.pw, in.ph}, bx - 4, by - 4, in.ral != 0, w);
#pragma unroll
      for (int r = 0; r < 12; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) a[r][k] = __builtin_amdgcn_alignbyte(w[r][k + 1], w[r][k], s0);
    } else {
#pragma unroll
      for (int r = 0; r < 12; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) a[r][k] = 0u;
    }
  }
  // stage 1 in the (s - 128) domain (UnitWin::pred): sum c.s - 8192
  template <int OX>
  __device__ __forceinline__ void hstage(int fx, int (&t)[12][4]) const {
    uint32_t hlo, hhi;
    luma_taps(fx, hlo, hhi);
#pragma unroll
    for (int r = 0; r < 12; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) {   // bytes c + OX .. c + OX + 7 of the row
        const int p = c + OX, q = c + OX + 4;
        const uint32_t b0 = (p & 3) ? __builtin_amdgcn_alignbyte(a[r][(p >> 2) + 1], a[r][p >> 2], (uint32_t)(p & 3)) : a[r][p >> 2];
        const uint32_t b1 = (q & 3) ? __builtin_amdgcn_alignbyte(a[r][(q >> 2) + 1], a[r][q >> 2], (uint32_t)(q & 3)) : a[r][q >> 2];
        t[r][c] = dot4(b1, hhi, dot4(b0, hlo, 0));
      }
  }
  // stage 2, uni-pred (isLast): (sum + 2048 + (8192 << 6)) >> 12 clipped
  static __device__ __forceinline__ int finish(int sum) { return clamp_i((sum + 2048 + (8192 << 6)) >> 12, 0, 255); }
};

template <>
struct SfWin<true> {
  int sv[12][12];   // s - 512
  __device__ __forceinline__ void load(const SfInfo& in, int bx, int by, bool valid) {
    const uint16_t* pl = reinterpret_cast<const uint16_t*>(in.ref);
#pragma unroll
    for (int r = 0; r < 12; r++)
#pragma unroll
      for (int c = 0; c < 12; c++) sv[r][c] = 0;
    if (!valid) return;
#pragma unroll
    for (int r = 0; r < 12; r++) {
      const gu16c* row = (const gu16c*)(pl + (size_t)clamp_i(by - 4 + r, 0, in.ph - 1) * in.rstride);
#pragma unroll
      for (int c = 0; c < 12; c++) sv[r][c] = (int)row[clamp_i(bx - 4 + c, 0, in.pw - 1)] - 512;
    }
  }
  // stage 1 at bit depth 10 (pred10): (sum c.s') >> 2
  template <int OX>
  __device__ __forceinline__ void hstage(int fx, int (&t)[12][4]) const {
    uint32_t hlo, hhi;
    luma_taps(fx, hlo, hhi);
    int tp[8];
#pragma unroll
    for (int k = 0; k < 8; k++) tp[k] = tap_of(hlo, hhi, k);
#pragma unroll
    for (int r = 0; r < 12; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) acc += tp[k] * sv[r][c + OX + k];
        t[r][c] = acc >> 2;
      }
  }
  // stage 2, uni-pred (isLast): ((sum + 512) >> 10) + 512 clipped
  static __device__ __forceinline__ int finish(int sum) { return clamp_i(((sum + 512) >> 10) + 512, 0, 1023); }
};

// What a lane needs to turn a unit's distortion into its group's sum in the job's LDS row.
struct SfLane {
  uint32_t* row;   // the job's dist[49] in LDS
  int G, lane, mode;
  bool valid;      // the lane has a unit this round
  bool store;      // the group's first lane
  bool lead8;      // the first lane of its 8x8 tile's quad
};

// The second stage at row offset OY (0: integer part -1, 1: integer part 0) and fraction fy, the
// unit's distortion against o, the group sum, and its addition to position idx.
template <bool k10, int OY>
__device__ __forceinline__ void sf_position(const int (&t)[12][4], int fy, const int (&o)[4][4], const SfLane& L, int idx) {
  uint32_t vlo, vhi;
  luma_taps(fy, vlo, vhi);
  int tp[8];
#pragma unroll
  for (int k = 0; k < 8; k++) tp[k] = tap_of(vlo, vhi, k);
  int d[4][4];
#pragma unroll
  for (int y = 0; y < 4; y++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += t[y + OY + k][c] * tp[k];
      d[y][c] = o[y][c] - SfWin<k10>::finish(sum);
    }
  // the lanes of a quad share a job and a round: the cross-lane stages of an 8x8 tile see all four
  uint32_t acc = unit_dist(d, L.mode, L.lane, L.lead8);
  if (!L.valid) acc = 0;
  acc = group_sum(acc, L.G, L.lane);   // wave-uniform control flow: every lane of the wave is here
  if (L.valid && L.store) L.row[idx] += acc;   // one writer per job: its group's first lane
}

// The seven dy of one dx: t holds the first stage of that dx.
template <bool k10>
__device__ __forceinline__ void sf_column(const int (&t)[12][4], const int (&o)[4][4], const SfLane& L, int dx) {
  for (int fy = 1; fy < 4; fy++) sf_position<k10, 0>(t, fy, o, L, surf_index(dx, fy - 4));
  for (int fy = 0; fy < 4; fy++) sf_position<k10, 1>(t, fy, o, L, surf_index(dx, fy));
}

template <bool k10>
__global__ __launch_bounds__(kSfBlock) void k_cost_surface(SurfArgs a) {
  __shared__ SfInfo info[kSfTasks];
  __shared__ __attribute__((aligned(16))) uint32_t out[kSfTasks * kSfWords];   // the jobs' fme_surface rows
  __shared__ uint8_t slot_task[kGroupSlots];   // job of each 4-lane slot
  __shared__ int total_lanes;
  const int t = (int)threadIdx.x, lane = t & 63;
  const int t0 = (int)blockIdx.x * kSfTasks;
  const int nt = min(kSfTasks, a.n - t0);   // jobs of this workgroup (> 0 by the grid)
  for (int i = t; i < kSfTasks * kSfWords; i += kSfBlock) out[i] = 0u;
  if (t < kSfTasks) {   // the first wave: one job per lane
    SfInfo& in = info[t];
    int lanes = 0;
    in.valid = 0;
    in.mode = kDistSad;
    in.uxn = 1;
    in.units = 0;
    if (t < nt) {
      const fme_job j = a.jobs[t0 + t];
      const unsigned p0 = a.probe ? a.probe[2 * (size_t)(t0 + t)] : FME_SURF_NO_PROBE;
      const unsigned p1 = a.probe ? a.probe[2 * (size_t)(t0 + t) + 1] : FME_SURF_NO_PROBE;
      in.probe0 = (int)p0;
      in.probe1 = (int)p1;
      if (!sf_job_valid(a, j, p0, p1)) {
        atomicAdd(a.invalid, 1);
      } else {
        const PicDesc p = a.pics[j.ref_id];
        in.valid = 1;
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
        in.ml = a.mlambda[j.lambda_id];
        in.x = j.x;
        in.y = j.y;
        in.w = j.w;
        in.uxn = j.w >> 2;
        const int units = (j.w >> 2) * (j.h >> 2);
        in.units = units;
        in.mvx = j.mv_x;
        in.mvy = j.mv_y;
        in.mvpx = j.mvp_x;
        in.mvpy = j.mvp_y;
        const bool had = a.use_hadamard && !(j.flags & FME_JOB_LOSSLESS);
        in.mode = dist_mode(had, j.w, j.h);
        lanes = group_lanes(units);
      }
    }
    in.lanes = lanes;
    in.start = pack_groups(lanes, lane, slot_task, total_lanes);
  }
  __syncthreads();
  const int total = total_lanes;
  for (int g0 = 0; g0 < total; g0 += kSfBlock) {   // workgroup-uniform
    const int g = g0 + t;
    const bool act = g < total;
    const int q = act ? (int)slot_task[g >> 2] : 0;
    const SfInfo& in = info[q];
    const int G = act ? in.lanes : 64;
    const int li = g - in.start;
    const int units = act ? in.units : 0;
    // a group of 64 lanes fills its wave, so the rounds of a wave's groups are 1 or all the same
    for (int u = li; __any(u < units); u += G) {   // wave-uniform
      const bool valid = u < units;
      const int mode = in.mode, uxn = max(in.uxn, 1);
      int ux, uy;
      unit_xy(u, uxn, mode == kDistHad8, ux, uy);
      const int x = in.x + 4 * ux, y = in.y + 4 * uy;
      SfWin<k10> win;
      win.load(in, x + in.mvx, y + in.mvy, valid);
      int o[4][4];
      unit_target<k10>(in, x, y, valid, o);   // fme_unit_target.h
      SfLane L;
      L.row = out + q * kSfWords;
      L.G = G;
      L.lane = lane;
      L.mode = mode;
      L.valid = valid;
      L.store = li == 0;
      L.lead8 = (u & 3) == 0;
      int tt[12][4];
      for (int fx = 1; fx < 4; fx++) {
        win.template hstage<0>(fx, tt);
        sf_column<k10>(tt, o, L, fx - 4);
      }
      for (int fx = 0; fx < 4; fx++) {
        win.template hstage<1>(fx, tt);
        sf_column<k10>(tt, o, L, fx);
      }
    }
  }
  __syncthreads();
  // the PU's sum >> bitDepth - 8, and the costs; an invalid job's words are all ones
  const int sh = k10 ? a.bit_depth - 8 : 0;
  for (int i = t; i < nt * FME_SURF_POINTS; i += kSfBlock) {
    const int q = i / FME_SURF_POINTS, idx = i - q * FME_SURF_POINTS;
    const SfInfo& in = info[q];
    uint32_t dist = kSurfNone, cost = kSurfNone;
    if (in.valid) {
      dist = out[q * kSfWords + idx] >> sh;
      cost = dist + mv_cost(in.ml, mv_bits(4 * in.mvx + surf_dx(idx), 4 * in.mvy + surf_dy(idx), 0, in.mvpx, in.mvpy));
    }
    out[q * kSfWords + idx] = dist;
    out[q * kSfWords + FME_SURF_POINTS + idx] = cost;
  }
  __syncthreads();
  if (a.pick && t < nt) {
    const SfInfo& in = info[t];
    fme_surface_pick p;
    if (in.valid) {
      surf_pick(out + t * kSfWords + FME_SURF_POINTS, (unsigned)in.probe0, (unsigned)in.probe1, p);
    } else {
      p.min_cost = p.probe_cost[0] = p.probe_cost[1] = kSurfNone;
      p.min_idx = 0xFF;
      p.probe[0] = (uint8_t)in.probe0;
      p.probe[1] = (uint8_t)in.probe1;
      p.status = 1;
    }
    sf_u4 v;
    v.x = p.min_cost;
    v.y = p.probe_cost[0];
    v.z = p.probe_cost[1];
    v.w = (uint32_t)p.min_idx | ((uint32_t)p.probe[0] << 8) | ((uint32_t)p.probe[1] << 16) | ((uint32_t)p.status << 24);
    *(g_sf_u4*)(a.pick + t0 + t) = v;
  }
  if (a.surf) {   // the workgroup's rows are contiguous: whole 16-byte stores, one 8-byte tail when nt is odd
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.surf + t0);
    const int words = nt * kSfWords;
    for (int v = t; v < (words >> 2); v += kSfBlock) {
      sf_u4 x;
      x.x = out[4 * v];
      x.y = out[4 * v + 1];
      x.z = out[4 * v + 2];
      x.w = out[4 * v + 3];
      *(g_sf_u4*)(dst + 4 * v) = x;
    }
    if ((words & 3) && t == 0) {
      sf_u2 x;
      x.x = out[words - 2];
      x.y = out[words - 1];
      *(g_sf_u2*)(dst + words - 2) = x;
    }
  }
}

}  // namespace

hipError_t launch_cost_surface(const SurfArgs& a, hipStream_t s) {
  return launch_by_depth(k_cost_surface<false>, k_cost_surface<true>, (a.n + kSfTasks - 1) / kSfTasks, kSfBlock, a, s);
}

}  // namespace fme
