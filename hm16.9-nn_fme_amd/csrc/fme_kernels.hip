// fme_kernels.hip — CDNA4 (gfx950) kernels of the fractional-pel motion-estimation path.
//
// One batch of PU jobs runs as three launches (front, search, nn_tail; the picture / lambda tables
// travel in the front end's kernel argument).  The
// jobs are read where the caller put them, through load_job (fme_device.h): fme_job rows, or the
// 16-byte fme_job_packed rows of the packed entry points expanded in registers; no kernel writes
// an unpacked copy.
//   front      per job: validation, PU-shape class, and for packed rows the keyed jobs' key
//              offsets (a scan per 64-job group from key_base); per block: the jobs grouped by
//              class straight into perm (class regions a fixed distance apart) and the max of the
//              NN "last writer" indices; the block that finishes last: the schedule from the class
//              totals (the search's tile ranges and per-XCD queues), the prefix-max of the writer
//              indices over the blocks, and the other counter block zeroed for the next batch,
//              which therefore needs no fill dispatch.
//              (The integer search keeps the two passes this replaced, k_classify and k_scatter:
//              its class offsets are dense and its schedule is built on the host.)
//   search     EMI square step + FracDIF per tile of same-shape PUs (fme_lane.hip, fme_lane10.hip).
//   nn_tail    prefix-max over jobs resolves which earlier job last wrote each array_e slot
//              (the reference's stale global state, TEncSearch.cpp:55-57, 198-201), then
//              NN_pred() (85-204) and the xMotionEstimation tail (4586-4597), one lane per job.
//
// Integer arithmetic follows TComInterpolationFilter (14-bit intermediate, offsets -8192 and
// 526336, shift 12) and TComRdCost (xGetHADs 8x8/4x4, SSE, SAD with FEN row subsampling).
// MV cost uses double like TComRdCost::getCost.  The NN is float32 with no contraction
// (this file is compiled with -ffp-contract=off) and sequential-k sums.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fme_device.h"
#include "fme_simd.h"

namespace fme {

// ---------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------
// HEVC luma taps (TComInterpolationFilter.cpp:57-63), selected without memory traffic.
__device__ __forceinline__ void luma_taps(int f, int (&c)[8]) {
  if (f == 1) {
    c[0] = -1; c[1] = 4; c[2] = -10; c[3] = 58; c[4] = 17; c[5] = -5; c[6] = 1; c[7] = 0;
  } else if (f == 2) {
    c[0] = -1; c[1] = 4; c[2] = -11; c[3] = 40; c[4] = 40; c[5] = -11; c[6] = 4; c[7] = -1;
  } else {
    c[0] = 0; c[1] = 1; c[2] = -5; c[3] = 17; c[4] = 58; c[5] = -10; c[6] = 4; c[7] = -1;
  }
}

// Candidate order of xPatternRefinement (s_acMvRefineH / s_acMvRefineQ, TEncSearch.cpp:212-236).
__device__ __forceinline__ int decode_offset(uint32_t code) { return code == 1 ? -1 : (code == 2 ? 1 : 0); }
// 2-bit code per index (0 -> 0, 1 -> -1, 2 -> +1), index 0 in the top pair of 18 bits.
__device__ __forceinline__ int refine_dx(int half, int i) {
  (void)half;  // x components of H9 and Q9 coincide
  return decode_offset((0x666u >> (2 * (8 - i))) & 3u);
}
__device__ __forceinline__ int refine_dy(int half, int i) {
  return decode_offset(((half ? 0x605au : 0x650au) >> (2 * (8 - i))) & 3u);
}

// ---------------------------------------------------------------------------------------
// class table helpers
// ---------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int class_of(int w, int h) {
  for (int c = 0; c < kNumClasses; c++)
    if (kClassW[c] == w && kClassH[c] == h) return c;
  return 255;
}

// ---------------------------------------------------------------------------------------
// classify: class histogram + first pass of the NN writer prefix-max
// ---------------------------------------------------------------------------------------
// PU shape -> class: [(w/4 - 1) * 16 + h/4 - 1], 255 = not an HEVC inter PU shape
struct ClassLut {
  uint8_t v[256];
  constexpr ClassLut() : v() {
    for (int i = 0; i < 256; i++) v[i] = 255;
    for (int c = 0; c < kNumClasses; c++) v[((kClassW[c] >> 2) - 1) * 16 + (kClassH[c] >> 2) - 1] = (uint8_t)c;
  }
};
__constant__ ClassLut kClassLut = ClassLut();

// What a workgroup holds in LDS to validate its jobs.
struct FrontTables {
  uint8_t lut[256];
  int32_t pic_w[FME_MAX_PICTURES], pic_h[FME_MAX_PICTURES];  // pic_w -1: slot unset
  int32_t keys_bad;
};
constexpr int kFrontQ = kJobsPerScanBlock / kBlock;   // jobs per lane: base + q * kBlock + tid

// A workgroup's jobs, every load issued before any is used (the front end is a few dependent memory
// latencies long).
__device__ __forceinline__ void front_load(const BatchArgs& a, const WorkBufs& w, int base, fme_job (&jb)[kFrontQ]) {
  const int tid = threadIdx.x;
  if (a.pjobs) {
    // Packed rows: a wave's 64 lanes hold one 64-job group (base and q * kBlock are multiples of
    // 64), whose keyed blocks follow key_base[group] densely in job order, so a job's key offset
    // is the base plus the exclusive sum of w*h over the group's earlier keyed jobs.  Groups
    // without a keyed job (every group of a uni-pred batch) scan and write nothing.
    job_u4 row[kFrontQ];
#pragma unroll
    for (int q = 0; q < kFrontQ; q++) {
      const int i = base + q * kBlock + tid;
      row[q] = job_u4{0u, 0u, 0u, 0u};
      if (i < a.n) row[q] = packed_row(a, i);
    }
#pragma unroll
    for (int q = 0; q < kFrontQ; q++) {
      const int i = base + q * kBlock + tid;
      const bool keyed_q = i < a.n && packed_keyed(row[q].y);
      int ko = -1;
      if (__ballot(keyed_q)) {   // wave-uniform
        const int wh = (int)((((row[q].x >> 22) & 15u) + 1u) * 4u) * (int)((((row[q].x >> 26) & 15u) + 1u) * 4u);
        const int lane = tid & 63;
        int s = keyed_q ? wh : 0;   // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(s, off, 64);
          if (lane >= off) s += o;
        }
        if (keyed_q) {
          ko = a.key_base[i >> 6] + s - wh;
          w.koff[i] = ko;
        }
      }
      jb[q] = expand_job(row[q], ko);
    }
  } else {
#pragma unroll
    for (int q = 0; q < kFrontQ; q++) {
      const int i = base + q * kBlock + tid;
      if (i < a.n) jb[q] = load_job(a, i);
    }
  }
}

// The class table, the picture sizes and the key flag, one entry per lane (before the workgroup's barrier).
// pics: the batch's picture table (PicDesc: the device copy; BatchPic: k_front's kernel argument).
template <class Pic>
__device__ __forceinline__ void front_tables(const BatchArgs& a, const Pic* pics, FrontTables& T) {
  const int tid = threadIdx.x;
  if (tid == 0) T.keys_bad = a.key_invalid ? *a.key_invalid : 0;
  T.lut[tid] = kClassLut.v[tid];
  if (tid < FME_MAX_PICTURES) {
    const Pic p = pics[tid];
    T.pic_w[tid] = p.luma ? p.width : -1;
    T.pic_h[tid] = p.height;
  }
}

// Job i's class; 255 for a shape that is no HEVC inter PU and for what would make the search read
// undefined memory.
__device__ __forceinline__ int front_class(const BatchArgs& a, const FrontTables& T, const fme_job& j, int i) {
  const int c = ((j.w | j.h) & 3) == 0 && j.w >= 4 && j.w <= 64 && j.h >= 4 && j.h <= 64
                    ? T.lut[((j.w >> 2) - 1) * 16 + (j.h >> 2) - 1] : 255;
  bool ok = j.ref_id < FME_MAX_PICTURES && j.lambda_id < FME_MAX_LAMBDAS && T.pic_w[j.ref_id] >= 0;
  if (ok) {
    if (j.key_offset >= 0) {
      ok = (int64_t)j.key_offset + (int64_t)j.w * j.h <= a.n_keys && T.keys_bad == 0;
    } else {
      ok = j.org_id < FME_MAX_PICTURES && T.pic_w[j.org_id] >= 0 &&
           (int)j.x + j.w <= T.pic_w[j.org_id] && (int)j.y + j.h <= T.pic_h[j.org_id];
    }
  }
  // FME_JOB_NN_IN: its input row must be bound (fme_set_nn_inputs)
  if ((j.flags & FME_JOB_NN_IN) && (!a.nn_in || i >= a.nn_in_cap)) ok = false;
  return ok ? c : 255;
}

// The NN "last writer" indices job i raises (first pass of the tail's prefix-max scan).
__device__ __forceinline__ void front_writers(const fme_job& j, int i, int (&mx)[9]) {
  if (!nn_writes_c(j)) return;
  const int np = nn_pushes(j);
#pragma unroll
  for (int s = 0; s < 8; s++)
    if (np > s) mx[s] = max(mx[s], i);
  mx[8] = max(mx[8], i);
}

// The integer search's first pass: class per job, the class histogram in w.counts.
__global__ __launch_bounds__(kBlock) void k_classify(BatchArgs a, WorkBufs w) {
  __shared__ FrontTables T;
  __shared__ int32_t hist[kNumClasses + 1];
  __shared__ int32_t agg[9];
  __shared__ int32_t keyed;
  const int tid = threadIdx.x;
  const int base = blockIdx.x * kJobsPerScanBlock;
  fme_job jb[kFrontQ];
  front_load(a, w, base, jb);
  front_tables(a, a.pics, T);
  if (tid == 0) keyed = 0;
  if (tid < kNumClasses + 1) hist[tid] = 0;
  if (tid < 9) agg[tid] = -1;
  __syncthreads();
  int mx[9];
#pragma unroll
  for (int f = 0; f < 9; f++) mx[f] = -1;
#pragma unroll
  for (int q = 0; q < kFrontQ; q++) {
    const int i = base + q * kBlock + tid;
    if (i < a.n) {
      const fme_job& j = jb[q];
      const int c = front_class(a, T, j, i);
      w.cls[i] = (uint8_t)c;
      atomicAdd(&hist[c == 255 ? kNumClasses : c], 1);
      if (j.key_offset >= 0) atomicAdd(&keyed, 1);
      front_writers(j, i, mx);
    }
  }
#pragma unroll
  for (int f = 0; f < 9; f++)
    if (mx[f] >= 0) atomicMax(&agg[f], mx[f]);
  __syncthreads();
  if (tid < kNumClasses + 1 && hist[tid]) atomicAdd(&w.counts[tid], hist[tid]);
  if (tid == 0 && keyed) atomicAdd(&w.counts[kKeyedWord], keyed);
  if (tid < 9) w.blk_agg[blockIdx.x * 9 + tid] = agg[tid];
}

// ---------------------------------------------------------------------------------------
// The schedule: class totals -> the search kernel's block ranges and the lane kernels' per-XCD tile
// queues, all on the device, so a batch needs no host round trip between the front end and the search.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_excl_scan(int v) {
  const int lane = (int)threadIdx.x & 63;
  int s = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(s, off, 64);
    if (lane >= off) s += o;
  }
  return s - v;
}

// One wave; lane c < kNumClasses holds class c's count (0 in every lane of a rejected batch, inv > 0).
// Returns class c's offset in perm: c * cap, or with cap = 0 the dense one (the counts' exclusive sum).
// publish: also write *sc (class offsets and counts, block ranges, XCD queues, the invalid count).
__device__ __forceinline__ int build_schedule(int cnt, int inv, const SchedParams& p, Schedule* sc, bool publish, int cap) {
  const int c = (int)threadIdx.x & 63;
  const int off = cap > 0 ? c * cap : wave_excl_scan(cnt);
  if (!publish) return off;   // wave-uniform
  const int nb = cnt > 0 ? (int)(((long long)cnt * p.lanes[c < kNumClasses ? c : 0] + 63) / 64) : 0;   // 64-lane wave tiles
  if (c < kNumClasses) {
    sc->class_off[c] = off;
    sc->class_cnt[c] = cnt;
  }
  {
    const int ex = wave_excl_scan(nb);
    if (c <= kNumClasses) sc->prefix[c] = ex;     // [kNumClasses] = the total
  }
  // per-XCD queues (Schedule::xq): band x of class c = its tiles [nb x / 8, nb (x+1) / 8)
  auto band_lo = [&](int B) { return (int)(((long long)nb * B) / 8); };
#pragma unroll 1
  for (int x = 0; x < 8; x++) {
    const int mine_c = c < kNumClasses ? band_lo(x + 1) - band_lo(x) : 0;   // class c's band tiles
    const int mine = __shfl(mine_c, c < kNumClasses ? lane_class_at(c) : c);  // position c's
    const int ex = wave_excl_scan(mine);
    if (c <= kNumClasses) sc->xq[x][c] = ex;
  }
  if (c == 0) sc->invalid = inv;
  return off;
}

// ---------------------------------------------------------------------------------------
// The front end of a refinement batch in one pass.  Every workgroup, for its 1,024 jobs: class and
// validation per job (cls), the jobs' ranks per class in call order (a ballot per class a wave
// holds, then a scan over the workgroup's 16 64-job segments: no atomic per job), its base in each
// class from one returning atomicAdd on the class cursor, and perm[c * perm_cap + base + rank] = i at
// once: the class regions of perm are perm_cap jobs apart, so no workgroup needs the totals.  The
// NN writer maxima go to blk_agg with write-through stores.  Once those and the atomics have been
// performed the workgroup draws a ticket; the workgroup that draws the last one (nobody waits or
// polls, so a workgroup that has not started holds nothing up) is the only one that reads other
// workgroups' data, after an agent-scope acquire and with agent-scope loads, as they ran on other
// XCDs: the class totals (the cursors' final values) become the Schedule, blk_agg's exclusive
// prefix-max over the scan blocks becomes blk_prefix (k_nn_tail's carry-in of the stale-state
// scan), and the other counter block is zeroed for the next batch, which therefore needs no fill
// dispatch.  What the kernel's 37 us are made of, step by step: DESIGN.md §5 "One-pass front end".
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int ld_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int32_t* p, int v) {   // a write-through store: past this XCD's L2
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// blk_prefix[b] = max of blk_agg[0 .. b) per field, for nb scan blocks, by one whole workgroup: each
// lane takes a contiguous run of blocks, the lanes' run maxima are scanned, each lane walks its run again.
// The loads go out four blocks (36 words) at a time before any is used: this is the one workgroup
// the whole kernel waits for.  A lane's run of up to four blocks (1,024 scan blocks, a 1080p frame
// has 843) stays in registers for the second walk.
constexpr int kPfxAhead = 4;
__device__ __forceinline__ void front_agg_load(const WorkBufs& w, int b, int b1, int (&v)[kPfxAhead][9]) {
#pragma unroll
  for (int k = 0; k < kPfxAhead; k++) {
#pragma unroll
    for (int f = 0; f < 9; f++) v[k][f] = b + k < b1 ? ld_agent(w.blk_agg + (b + k) * 9 + f) : -1;
  }
}
__device__ __forceinline__ void front_blk_prefix(const WorkBufs& w, int nb) {
  __shared__ int32_t red[kBlock / 64][9];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per = (nb + kBlock - 1) / kBlock;
  const int b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
  int m[9], v[kPfxAhead][9];
#pragma unroll
  for (int f = 0; f < 9; f++) m[f] = -1;
  for (int b = b0; b < b1 || b == b0; b += kPfxAhead) {   // (once at least: v is the lane's run when per <= kPfxAhead)
    front_agg_load(w, b, b1, v);
#pragma unroll
    for (int k = 0; k < kPfxAhead; k++) {
#pragma unroll
      for (int f = 0; f < 9; f++) m[f] = max(m[f], v[k][f]);
    }
  }
  int run[9];   // the maxima of the lanes before this one: inclusive scan, then shifted by one lane
#pragma unroll
  for (int f = 0; f < 9; f++) {
    int s = m[f];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(s, off, 64);
      if (lane >= off) s = max(s, o);
    }
    if (lane == 63) red[wv][f] = s;
    const int e = __shfl_up(s, 1, 64);
    run[f] = lane ? e : -1;
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 9; f++)
    for (int q = 0; q < wv; q++) run[f] = max(run[f], red[q][f]);
  for (int b = b0; b < b1; b += kPfxAhead) {
    if (per > kPfxAhead) front_agg_load(w, b, b1, v);
#pragma unroll
    for (int k = 0; k < kPfxAhead; k++) {
      if (b + k < b1) {
#pragma unroll
        for (int f = 0; f < 9; f++) {
          w.blk_prefix[(b + k) * 9 + f] = run[f];
          run[f] = max(run[f], v[k][f]);
        }
      }
    }
  }
}

// The batch's picture / lambda tables are the kernel argument tab (2 KB: fme_device.h BatchTables;
// with the other arguments and the hidden ones 2.6 KB of the 4 KB argument segment, checked
// below): every workgroup validates against the argument, so none waits for the device copy, and
// the first workgroup writes that copy (d_pics, d_ml: the batch's ring entry) for the search and
// the tail, which follow in stream order.  No launch of its own carries the tables (k_put_tables
// did: one workgroup that queued for a wave slot behind the search before the front end could
// follow it).
static_assert(sizeof(BatchArgs) + sizeof(WorkBufs) + sizeof(SchedParams) + sizeof(BatchTables) + 2 * sizeof(void*) + 256 <= 4096,
              "k_front's arguments and the 256 hidden bytes must fit the 4 KB kernel-argument segment");
static_assert(FME_MAX_PICTURES <= kBlock && FME_MAX_LAMBDAS <= kBlock, "one lane per table entry");
__global__ __launch_bounds__(kBlock) void k_front(BatchArgs a, WorkBufs w, SchedParams sp, BatchTables tab,
                                                  PicDesc* __restrict__ d_pics, double* __restrict__ d_ml) {
  constexpr int kSeg = kFrontQ * (kBlock / 64);   // 64-job segments of the workgroup, in call order
  __shared__ FrontTables T;
  __shared__ int32_t seg[kSeg][kNumClasses + 1];  // jobs per class ([kNumClasses]: invalid), then their exclusive sums
  __shared__ int32_t basep[kNumClasses];
  __shared__ int32_t agg[9];
  __shared__ int32_t keyed, last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int base = blockIdx.x * kJobsPerScanBlock;
  fme_job jb[kFrontQ];
  front_load(a, w, base, jb);
  front_tables(a, tab.pics, T);
  if (blockIdx.x == 0) {
    if (tid < FME_MAX_PICTURES) {
      const BatchPic p = tab.pics[tid];
      d_pics[tid] = PicDesc{p.luma, p.stride, p.width, p.height, nullptr, nullptr, 0, 0};
    }
    if (tid < FME_MAX_LAMBDAS) d_ml[tid] = tab.ml[tid];
  }
  if (tid == 0) keyed = 0;
  for (int k = tid; k < kSeg * (kNumClasses + 1); k += kBlock) (&seg[0][0])[k] = 0;
  if (tid < 9) agg[tid] = -1;
  __syncthreads();
  int mx[9], cls[kFrontQ], rank[kFrontQ];
#pragma unroll
  for (int f = 0; f < 9; f++) mx[f] = -1;
  int nkeyed = 0;
#pragma unroll
  for (int q = 0; q < kFrontQ; q++) {
    const int i = base + q * kBlock + tid;
    const bool valid = i < a.n;
    cls[q] = kNumClasses;
    rank[q] = 0;
    if (valid) {
      const fme_job& j = jb[q];
      const int c = front_class(a, T, j, i);
      w.cls[i] = (uint8_t)c;
      cls[q] = c == 255 ? kNumClasses : c;
      front_writers(j, i, mx);
    }
    nkeyed += __popcll(__ballot(valid && jb[q].key_offset >= 0));
    // ranks inside the wave's segment: one ballot per class the segment holds
    int32_t* sg = seg[q * (kBlock / 64) + (tid >> 6)];
    unsigned long long rem = __ballot(valid);
    while (rem) {   // wave-uniform
      const int cl = __shfl(cls[q], __ffsll((long long)rem) - 1);
      const unsigned long long m = __ballot(valid && cls[q] == cl);
      if (valid && cls[q] == cl) {
        rank[q] = __popcll(m & ((1ull << lane) - 1ull));
        if (rank[q] == 0) sg[cl] = __popcll(m);
      }
      rem &= ~m;
    }
  }
  if (lane == 0 && nkeyed) atomicAdd(&keyed, nkeyed);
  // the wave's maxima first: 64 lanes' atomics on one LDS word are served one after the other
#pragma unroll
  for (int f = 0; f < 9; f++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx[f] = max(mx[f], __shfl_xor(mx[f], off));
  }
  if (lane < 9) {
    int v = mx[0];
#pragma unroll
    for (int f = 1; f < 9; f++) v = lane == f ? mx[f] : v;
    if (v >= 0) atomicMax(&agg[lane], v);
  }
  __syncthreads();
  if (tid < kNumClasses + 2) {
    // one atomic instruction per workgroup, all in one 128-byte line (fme_device.h, counter block):
    // lanes 0..23 the class cursors, whose old values are the workgroup's bases; lanes 24, 25 the
    // invalid and keyed counts
    int tot = keyed;
    if (tid < kNumClasses + 1) {
      tot = 0;
      for (int s = 0; s < kSeg; s++) {
        const int t = seg[s][tid];
        seg[s][tid] = tot;
        tot += t;
      }
    }
    const int old = tot ? atomicAdd(&w.cursor[tid], tot) : 0;
    if (tid < kNumClasses) basep[tid] = old;
  } else if (tid >= 64 && tid < 64 + 9) {
    st_agent(w.blk_agg + blockIdx.x * 9 + tid - 64, agg[tid - 64]);
  }
  // What the last workgroup reads of this one went out as agent-scope atomics and write-through
  // stores; every wave waits until its own have been performed, then lane 0 draws the ticket.  (An
  // agent-scope release fence here instead writes the XCD's L2 back once per workgroup, with the
  // other workgroups' perm and cls stores in it: 8 us more per batch)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = __hip_atomic_fetch_add(&w.counts[kTicketWord], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
#pragma unroll
  for (int q = 0; q < kFrontQ; q++) {
    const int i = base + q * kBlock + tid;
    const int c = cls[q];
    if (c < kNumClasses)   // (jobs past a.n hold kNumClasses)
      w.perm[(size_t)c * w.perm_cap + basep[c] + seg[q * (kBlock / 64) + (tid >> 6)][c] + rank[q]] = i;
  }
  __syncthreads();
  if (!last) return;
  // ---- the last workgroup: every other one has released its counts and blk_agg ----
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  int inv = 0, tot = 0;   // wave 0: the totals, asked for before the prefix pass and used after it
  if (tid < 64) {
    inv = ld_agent(w.cursor + kNumClasses);
    tot = tid < kNumClasses ? ld_agent(w.cursor + tid) : 0;
  } else if (tid < 64 + kCountWords) {
    w.counts_next[tid - 64] = 0;   // the next batch's counter block (also when this one is rejected)
  }
  front_blk_prefix(w, (int)gridDim.x);
  if (tid < 64) build_schedule(inv == 0 ? tot : 0, inv, sp, w.sched, true, w.perm_cap);
}

// ---------------------------------------------------------------------------------------
// The integer search's second pass: the class histogram -> dense class offsets (every block, one
// wave, one lane per class) and the jobs grouped by class (block-aggregated atomics).  Block 0 also
// writes the Schedule and zeroes the other counter block, as it did when refinement batches ran
// through this kernel; the integer search reads neither.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_scatter(BatchArgs a, WorkBufs w, SchedParams sp) {
  __shared__ int32_t cnt[kNumClasses], basep[kNumClasses], class_off[kNumClasses];
  const int tid = threadIdx.x;
  const int base = blockIdx.x * kJobsPerScanBlock;
  int rank[kJobsPerScanBlock / kBlock];
  int cls[kJobsPerScanBlock / kBlock];
#pragma unroll
  for (int q = 0; q < kJobsPerScanBlock / kBlock; q++) {
    const int i = base + q * kBlock + tid;
    cls[q] = 255;
    if (i < a.n) cls[q] = w.cls[i];
  }
  if (tid < 64) {
    const int inv = w.counts[kNumClasses];
    const int off = build_schedule((tid < kNumClasses && inv == 0) ? w.counts[tid] : 0, inv, sp, w.sched, blockIdx.x == 0, 0);
    if (tid < kNumClasses) class_off[tid] = off;
  } else if (blockIdx.x == 0 && tid < 64 + kCountWords) {
    w.counts_next[tid - 64] = 0;
  }
  if (w.counts[kNumClasses]) return;   // rejected batch: nothing downstream reads the grouping
  if (tid < kNumClasses) cnt[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kJobsPerScanBlock / kBlock; q++)
    if (cls[q] < kNumClasses) rank[q] = atomicAdd(&cnt[cls[q]], 1);
  __syncthreads();
  if (tid < kNumClasses) basep[tid] = cnt[tid] ? atomicAdd(&w.cursor[tid], cnt[tid]) : 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kJobsPerScanBlock / kBlock; q++) {
    const int i = base + q * kBlock + tid;
    if (cls[q] < kNumClasses) w.perm[class_off[cls[q]] + basep[cls[q]] + rank[q]] = i;
  }
}

// ---------------------------------------------------------------------------------------
// NN_pred() + xMotionEstimation tail, one lane per job.
// ---------------------------------------------------------------------------------------
enum {
  P_EMB0 = 0, P_EMB1 = 32, P_W1 = 64, P_W2 = 438, P_W3 = 878, P_B1 = 1858, P_G1 = 1880,
  P_BE1 = 1902, P_B2 = 1924, P_G2 = 1944, P_BE2 = 1964, P_BOUT = 1984, P_GIN = 2033,
  P_MEAN = 2042, P_STD = 2051
};


// Device layout of the net for the tail (built once per weight load by nn_pack, fme_device.h
// kNnPk*): rows paired for packed f32 math (row r in .x, row r+1 in .y, so both halves run
// the reference's sequential k order), and the 8 embedding terms of layer 1 folded into a
// per-PU-shape prefix: the partial sums after k = 0..7 depend only on (PUHeight, PUWidth).
void nn_pack(const float* P, float* Q) {
  for (int i = 0; i < kNnPkFloats; i++) Q[i] = 0.0f;
  for (int rh = 0; rh < 8; rh++)
    for (int rw = 0; rw < 8; rw++)
      for (int r = 0; r < 22; r++) {
        float s = 0.0f;   // TEncSearch.cpp:120 row r, terms k = 0..7 (embeddings), in order
        for (int k = 0; k < 4; k++) s = s + P[P_W1 + r * 17 + k] * P[P_EMB0 + rh * 4 + k];
        for (int k = 0; k < 4; k++) s = s + P[P_W1 + r * 17 + 4 + k] * P[P_EMB1 + rw * 4 + k];
        Q[kNnPkPfx + (rh * 8 + rw) * 22 + r] = s;
      }
  for (int r = 0; r < 22; r++)
    for (int k = 0; k < 9; k++) Q[kNnPkW1 + ((r / 2) * 9 + k) * 2 + (r & 1)] = P[P_W1 + r * 17 + 8 + k];
  for (int r = 0; r < 20; r++)
    for (int k = 0; k < 22; k++) Q[kNnPkW2 + ((r / 2) * 22 + k) * 2 + (r & 1)] = P[P_W2 + r * 22 + k];
  for (int r = 0; r < 49; r++)
    for (int k = 0; k < 20; k++) Q[kNnPkW3 + ((r / 2) * 20 + k) * 2 + (r & 1)] = P[P_W3 + r * 20 + k];
  for (int r = 0; r < 22; r++) {
    Q[kNnPkB1 + r] = P[P_B1 + r];
    Q[kNnPkG1 + r] = P[P_G1 + r];
    Q[kNnPkBE1 + r] = P[P_BE1 + r];
  }
  for (int r = 0; r < 20; r++) {
    Q[kNnPkB2 + r] = P[P_B2 + r];
    Q[kNnPkG2 + r] = P[P_G2 + r];
    Q[kNnPkBE2 + r] = P[P_BE2 + r];
  }
  for (int r = 0; r < 49; r++) Q[kNnPkBout + r] = P[P_BOUT + r];
  for (int k = 0; k < 9; k++) {
    Q[kNnPkGin + k] = P[P_GIN + k];
    Q[kNnPkMean + k] = P[P_MEAN + k];
    Q[kNnPkStd + k] = P[P_STD + k];
  }
}


// NN_pred() (TEncSearch.cpp:85-134) on the packed layout: float32, every dot product summed in
// k order without contraction (the sequential-k contract), BN as x*g + b.  The
// weights are wave-uniform, so they stream through the scalar cache into SGPR operands.
__device__ __forceinline__ int nn_forward(const float* __restrict__ Q, const uint32_t (&e)[8], uint32_t c, int pu_h,
                                          int pu_w) {
  const int t = emb_row_h(pu_h) * 8 + emb_row_w(pu_w);
  float in[9];
  const uint32_t raw[9] = {e[0], e[1], e[2], e[3], c, e[4], e[5], e[6], e[7]};
#pragma unroll
  for (int k = 0; k < 9; k++) {
    float v = (float)raw[k];
    v = (v - Q[kNnPkMean + k]) / Q[kNnPkStd + k];
    in[k] = v * Q[kNnPkGin + k];
  }
  const float* pfx = Q + kNnPkPfx + t * 22;
  f2 x1[11];
#pragma unroll
  for (int rp = 0; rp < 11; rp++) {
    f2 s = {pfx[2 * rp], pfx[2 * rp + 1]};
#pragma unroll
    for (int k = 0; k < 9; k++) s = s + ld2(Q, kNnPkW1 + (rp * 9 + k) * 2) * (f2){in[k], in[k]};
    s = relu2(s + ld2(Q, kNnPkB1 + 2 * rp));
    x1[rp] = s * ld2(Q, kNnPkG1 + 2 * rp) + ld2(Q, kNnPkBE1 + 2 * rp);
  }
  f2 x2[10];
#pragma unroll
  for (int rp = 0; rp < 10; rp++) {
    f2 s = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 22; k++) {
      const float xk = (k & 1) ? x1[k / 2].y : x1[k / 2].x;
      s = s + ld2(Q, kNnPkW2 + (rp * 22 + k) * 2) * (f2){xk, xk};
    }
    s = relu2(s + ld2(Q, kNnPkB2 + 2 * rp));
    x2[rp] = s * ld2(Q, kNnPkG2 + 2 * rp) + ld2(Q, kNnPkBE2 + 2 * rp);
  }
  int best = 0;
  float bv = 0.0f;
#pragma unroll 1   // the weights of one row pair per iteration (scalar loads, few SGPRs)
  for (int rp = 0; rp < 25; rp++) {
    f2 s = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 20; k++) {
      const float xk = (k & 1) ? x2[k / 2].y : x2[k / 2].x;
      s = s + ld2(Q, kNnPkW3 + (rp * 20 + k) * 2) * (f2){xk, xk};
    }
    s = s + ld2(Q, kNnPkBout + 2 * rp);
    // Eigen maxCoeff: first index of the maximum (strict >), rows in order
    if (rp == 0 || s.x > bv) {
      bv = s.x;
      best = 2 * rp;
    }
    if (rp < 24 && s.y > bv) {
      bv = s.y;
      best = 2 * rp + 1;
    }
  }
  return best;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// NN_pred() on the inputs job i sees + the xMotionEstimation tail (TEncSearch.cpp:4583-4597):
// src = the last writer of each carried field (writer_scan), r0..r3 = the job's 64-byte record.
__device__ __forceinline__ void tail_job(const BatchArgs& a, const WorkBufs& w, const float* __restrict__ nnp_g,
                                         int state_in, int i, const fme_job& j, const int (&src)[9], u32x4 r0,
                                         u32x4 r1, u32x4 r2, u32x4 r3) {
  const uint32_t* st_in = w.nn_state + 12 * state_in;
  uint32_t* st_out = w.nn_state + 12 * (state_in ^ 1);
  fme_result* r = a.res + i;
  const fme_result* sr = search_rec(a, w, i);
  const double ml = a.mlambda[j.lambda_id];
  const int mvx = (int16_t)(r0.x & 0xFFFF), mvy = (int16_t)(r0.x >> 16);
  const uint32_t own_emi[8] = {r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z};
  const uint32_t own_c = r1.z, own_n_emi = r3.w & 0xFF, frac_cost = r0.w;
  int offx, offy, cls = 255;
  uint16_t status = 0;
  if (a.nn_mode) {
    NnCarried v;
    nn_carried(a, w, st_in, i, j, src, own_emi, own_c, false, v);
    cls = nn_forward(nnp_g, v.e, v.c, (int)v.ph, (int)v.pw);
    status = (uint16_t)nn_carried_status(nn_writes_c(j), own_n_emi, v);
    offx = cls % 7 - 3;
    offy = cls / 7 - 3;
    if (i == a.n - 1) nn_carry_on(st_out, v);
  } else {
    const int8_t hx = (int8_t)(r0.z & 0xFF), hy = (int8_t)((r0.z >> 8) & 0xFF);
    const int8_t qx = (int8_t)((r0.z >> 16) & 0xFF), qy = (int8_t)(r0.z >> 24);
    offx = 2 * hx + qx;
    offy = 2 * hy + qy;
  }
  const int fx = 4 * mvx + offx, fy = 4 * mvy + offy;
  uint32_t bits;
  const uint32_t cost = me_tail(j, ml, frac_cost, fx, fy, bits);
  store_outputs(r, sr, w.mv_out, i, fx, fy, cost, bits, (uint8_t)cls, status);
}

// One lane per job, one wave per workgroup, every wave on its own: the last-writer scan reads the
// earlier jobs of the wave's 1024-job scan block (kJobsPerScanBlock, the granularity of k_scatter's
// carry-in) again instead of meeting the block's other waves at a barrier, so a SIMD takes its next
// wave whenever one ends.  Until round 8 a workgroup held a whole scan block (one per CU at 4
// waves/SIMD, 843 of them on 256 CUs, the 16 waves in step through loads, scan, net and stores).
// A/B on the 1080p batch (tools/ab_bench.py, identical results, profiles/r08_ab.log): that form
// 0.110 ms; this one 0.091, the same with 128, 256 or 512 lanes per workgroup; at 6 waves/SIMD
// (73 VGPRs) 0.097.  The net is ≈ 3,100 instructions per wave, 1,640 of them packed f32 multiply /
// add in the reference's k order.  The packed forms issue in ≈ 4 cycles, plain v_mul_f32 /
// v_add_f32 in ≈ 2.2 (profiles/r08_valu_rate.txt), so a row pair costs the same either way: the
// pairs as scalar chains (91 VGPRs) ran 0.113 ms against 0.110 in the scan-block form.
constexpr int kTailNT = 64;

__global__ __launch_bounds__(kTailNT) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_nn_tail(BatchArgs a, WorkBufs w, const float* __restrict__ nnp_g, int state_in) {
  const int wbase = (int)blockIdx.x * kTailNT;   // the wave's first job (< a.n by the grid)
  const int i = wbase + (int)threadIdx.x;
  const bool valid = i < a.n;
  if (w.sched->invalid) {
    if (valid) reject_job(a, w, i, state_in);
    return;
  }
  fme_job j{};
  // the job and its 64-byte record, issued before the scan (the NN inputs are usually the job's
  // own pushes)
  u32x4 r0{}, r1{}, r2{}, r3{};
  if (valid) {
    j = load_job(a, i);
    const u32x4* rb = reinterpret_cast<const u32x4*>(search_rec(a, w, i));
    r0 = rb[0];
    r1 = rb[1];
    r2 = rb[2];
    r3 = rb[3];
  }
  // writer indices of this job (slots it pushes, C / PU size)
  int run[9];
  {
    const bool wr = valid && nn_writes_c(j);
    const int np = wr ? nn_pushes(j) : 0;
#pragma unroll
    for (int s = 0; s < 8; s++) run[s] = (np > s) ? i : -1;
    run[8] = wr ? i : -1;
  }
  int src[9];
  writer_scan_wave(a, run, w.blk_prefix + (wbase / kJobsPerScanBlock) * 9, wbase, src);
  if (valid) tail_job(a, w, nnp_g, state_in, i, j, src, r0, r1, r2, r3);
}


// ---------------------------------------------------------------------------------------
// host launch helpers
// ---------------------------------------------------------------------------------------
static int nblocks(int n) { return (n + kJobsPerScanBlock - 1) / kJobsPerScanBlock; }

hipError_t launch_front(const BatchArgs& a, const WorkBufs& w, const SchedParams& p, const BatchTables& t,
                        PicDesc* d_pics, double* d_ml, hipStream_t s) {
  hipLaunchKernelGGL(k_front, dim3(nblocks(a.n)), dim3(kBlock), 0, s, a, w, p, t, d_pics, d_ml);
  return hipGetLastError();
}

hipError_t launch_classify(const BatchArgs& a, const WorkBufs& w, hipStream_t s) {
  hipLaunchKernelGGL(k_classify, dim3(nblocks(a.n)), dim3(kBlock), 0, s, a, w);
  return hipGetLastError();
}

// fme_nn_reset_state / fme_nn_set_state, applied in stream order: the 12 words travel as a
// kernel argument, so the host copy is free as soon as the launch returns.
struct State12 {
  uint32_t v[12];
};
__global__ void k_put_state(uint32_t* dst, State12 st) {
  if (threadIdx.x < 12) dst[threadIdx.x] = st.v[threadIdx.x];
}

// The picture / lambda tables for everything but a refinement batch, from a pinned, device-mapped
// host slot (fme_api.cpp sync_tables: a ring of slots, each reused only once its launch has run).
// (A refinement batch carries them in k_front's argument instead, to save this launch.)
__global__ __launch_bounds__(256) void k_put_tables(PicDesc* __restrict__ pics, double* __restrict__ ml,
                                                    const TablesSlot* __restrict__ t) {
  const int i = threadIdx.x;
  if (i < FME_MAX_PICTURES) pics[i] = t->pics[i];
  if (i < FME_MAX_LAMBDAS) ml[i] = t->ml[i];
}

hipError_t launch_put_tables(PicDesc* d_pics, double* d_ml, const TablesSlot* t_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_put_tables, dim3(1), dim3(256), 0, s, d_pics, d_ml, t_dev);
  return hipGetLastError();
}

hipError_t launch_put_state(uint32_t* dst, const uint32_t* v12, hipStream_t s) {
  State12 st;
  for (int k = 0; k < 12; k++) st.v[k] = v12[k];
  hipLaunchKernelGGL(k_put_state, dim3(1), dim3(64), 0, s, dst, st);
  return hipGetLastError();
}

hipError_t launch_scatter(const BatchArgs& a, const WorkBufs& w, const SchedParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_scatter, dim3(nblocks(a.n)), dim3(kBlock), 0, s, a, w, p);
  return hipGetLastError();
}

SchedParams sched_params() {
  SchedParams p{};
  for (int c = 0; c < kNumClasses; c++) p.lanes[c] = lane_lanes_per_pu(c);
  return p;
}

int cu_count(int device) {
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
  return v;
}

// ---------------------------------------------------------------------------------------
// results download: device rows -> pinned host memory, few workgroups.  Each lane keeps four
// 16-byte loads in flight, then stores them non-temporally: the rows go to the PCIe write path
// without allocating in L2.  tools/probes/d2h_kernel_probe.hip (profiles/r05_ab.log): PCIe write
// bound at ~54 GB/s from 8 workgroups of 256 lanes with nt stores (0.264 ms per 13.8 MB), where
// system-scope sc0 sc1 stores need 64 workgroups and one-wave groups 128.
// ---------------------------------------------------------------------------------------
constexpr int kDlThreads = 256;
__device__ __forceinline__ void dl_store(u32x4* p, u32x4 v) { __builtin_nontemporal_store(v, p); }
__global__ __launch_bounds__(kDlThreads) void k_download(const u32x4* __restrict__ src, u32x4* dst, long n16) {
  const long stride = (long)gridDim.x * kDlThreads;
  long i = (long)blockIdx.x * kDlThreads + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const u32x4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dl_store(dst + i, a);
    dl_store(dst + i + stride, b);
    dl_store(dst + i + 2 * stride, c);
    dl_store(dst + i + 3 * stride, d);
  }
  for (; i < n16; i += stride) dl_store(dst + i, src[i]);
}

__global__ __launch_bounds__(kBlock) void k_gather_jobs(const fme_job* __restrict__ src,
                                                       const fme_tz_ext* __restrict__ src_ext,
                                                       const int32_t* __restrict__ idx, fme_job* __restrict__ dst,
                                                       fme_tz_ext* __restrict__ dst_ext, int n) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const int u = idx[q];
  dst[q] = src[u];
  if (dst_ext) dst_ext[q] = src_ext[u];
}

hipError_t launch_gather_jobs(const fme_job* src, const fme_tz_ext* src_ext, const int32_t* idx, fme_job* dst,
                              fme_tz_ext* dst_ext, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather_jobs, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, src, src_ext, idx, dst,
                     dst_ext, n);
  return hipGetLastError();
}

hipError_t launch_download(const void* src, void* dst, size_t n16, int wgs, hipStream_t s) {
  const long need = (long)((n16 + kDlThreads - 1) / kDlThreads);
  const int g = (int)std::min<long>(wgs, std::max<long>(need, 1));
  hipLaunchKernelGGL(k_download, dim3(g), dim3(kDlThreads), 0, s, static_cast<const u32x4*>(src),
                     static_cast<u32x4*>(dst), (long)n16);
  return hipGetLastError();
}

hipError_t launch_nn_tail(const BatchArgs& a, const WorkBufs& w, const float* nn_params,
                          int state_in, hipStream_t s) {
  const int nb = (a.n + kTailNT - 1) / kTailNT;
  hipLaunchKernelGGL(k_nn_tail, dim3(nb), dim3(kTailNT), 0, s, a, w, nn_params, state_in);
  return hipGetLastError();
}

}  // namespace fme
