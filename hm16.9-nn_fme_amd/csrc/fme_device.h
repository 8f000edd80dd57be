// fme_device.h — types shared by the HIP kernels (fme_kernels.hip) and the host runtime
// (fme_api.cpp, fme_producers.cpp).  Not part of the public ABI (include/fme.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fme.h"
#include "../../include/fme_direct.h"
#include "../../include/fme_extern.h"
#include "../../include/fme_merge.h"
#include "../../include/fme_skip.h"
#include "../../include/fme_surface.h"
#include "fme_simd.h"
#include "fme_srv_pack.h"

namespace fme {

constexpr int kNumClasses = 24;      // HEVC inter PU shapes 4x8 .. 64x64 incl. AMP

// Order in which an XCD's band visits the PU classes (Schedule::xq position -> class id):
// 0 = by class id (smallest PUs first), 1 = reversed (largest first), 2 = smallest and largest
// alternating (0, 23, 1, 22, ...).  A/B on the 1080p batch: 0.876 / 0.880 / 0.884 ms, results
// identical (profiles/r06_ab.log): the band's first class pays its cold start whichever it is.
// Orders 0 and 1 both end with a class whose tiles are among the longest (64x64, 4x8).  An order
// with the costly classes first and the cheapest last (64x64, 48x64, 64x48, 4x8, 4x16, 8x4, then
// by falling cycles per tile of profiles/r06_lane_phase_stamps.txt) was built in round 13 and
// removed again: in the overlapped layout its headline runs fell into two groups, 1.020 - 1.039
// and 1.061 - 1.072 ms per step, against 1.018 - 1.042 for order 0 (profiles/r13_bench_headline.txt).
#ifndef FME_LANE_ORDER
#define FME_LANE_ORDER 0
#endif
__host__ __device__ __forceinline__ constexpr int lane_class_at(int pos) {
  return FME_LANE_ORDER == 1 ? kNumClasses - 1 - pos
         : FME_LANE_ORDER == 2 ? ((pos & 1) ? kNumClasses - 1 - (pos >> 1) : (pos >> 1))
                               : pos;
}
constexpr int kBlock = 256;          // threads per workgroup (4 wavefronts)
constexpr int kJobsPerScanBlock = 1024;  // classify / NN kernels: 4 jobs per thread
// One counter block, three 128-byte lines; a context holds two, used by alternate batches.
//   line 0: the integer search's class histogram (k_classify: 24 counts, [24] invalid jobs), its
//           keyed-job count, and k_front's done ticket
//   line 1: the 24 scatter cursors, then k_front's invalid and keyed counts: what a k_front
//           workgroup adds to with its one atomic instruction
//   line 2: the lane kernels' 8 tile-queue heads
// k_front's two atomic instructions per workgroup (cursors, ticket) go to two lines, and the
// cursors' instruction to one line only (DESIGN.md §5 "One-pass front end").
constexpr int kKeyedWord = 25;           // counts[]: jobs that read a key block (k_classify)
constexpr int kTicketWord = 28;          // counts[]: k_front's workgroups that are done (the last one builds the schedule)
constexpr int kCursorWord = 32;          // counts[]: WorkBufs::cursor; [kNumClasses], [kNumClasses + 1]: k_front's invalid / keyed jobs
constexpr int kTileCtrWord = 64;
constexpr int kCountWords = 96;
static_assert(kNumClasses < kKeyedWord && kKeyedWord < kTicketWord && kTicketWord < 32 && kCursorWord + kNumClasses + 2 <= 64 &&
                  kTileCtrWord + 8 <= kCountWords, "counter block");

// PU shape of each class (W, H).  Order: by area, then width.
constexpr int kClassW[kNumClasses] = {4, 8, 8, 4, 16, 8, 16, 12, 16, 16, 8, 32,
                                      16, 32, 24, 32, 32, 16, 64, 32, 64, 48, 64, 64};
constexpr int kClassH[kNumClasses] = {8, 4, 8, 16, 4, 16, 8, 16, 12, 16, 32, 8,
                                      32, 16, 32, 24, 32, 64, 16, 64, 32, 64, 48, 64};

struct PicDesc {
  const uint8_t* luma;
  int32_t stride, width, height;
  const uint8_t* cb;          // 4:2:0 chroma (motion compensation only); null when unset
  const uint8_t* cr;
  int32_t cstride;
  int32_t pad_;
};

// The launch of a kernel that is built per bit depth (template <bool k10>): the 10-bit instance
// when the arguments say so, nothing when there is no work.
template <class Args>
inline hipError_t launch_by_depth(void (*k8)(Args), void (*k10)(Args), int grid, int block, const Args& a,
                                  hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(a.bit_depth > 8 ? k10 : k8, dim3(grid), dim3(block), 0, s, a);
  return hipGetLastError();
}

// One motion-compensation launch (fme_mc.hip).
struct McArgs {
  const fme_mc_job* jobs;
  const PicDesc* pics;
  uint8_t* y;
  uint8_t* cb;
  uint8_t* cr;
  int32_t* invalid;           // count of skipped jobs
  int32_t n, y_stride, c_stride, width, height;
  int32_t bit_depth;          // 8, or 10: y / cb / cr and the pictures hold uint16 samples (strides in samples)
  const fme_wp_param* wp;     // [2][FME_MAX_PICTURES][3] weighted-prediction parameters (FME_MC_WP jobs)
};
hipError_t launch_mc(const McArgs& a, hipStream_t s);

// xGetTemplateCost's distortion (fme_mc.hip): SAD of the uni-pred luma prediction at one AMVP
// candidate (clipMv'd against the CU origin) against the original, one task per wave.
struct AmvpTask {
  uint16_t x, y;
  uint8_t w, h, org_id, ref_id;
  uint16_t cu_x, cu_y;
  int16_t mv_x, mv_y;
};
static_assert(sizeof(AmvpTask) == 16, "AmvpTask layout");
struct AmvpArgs {
  const AmvpTask* tasks;
  const PicDesc* pics;
  uint32_t* sad;
  int32_t n;
  int32_t bit_depth;          // 8, or 10: uint16 planes (k_amvp_sad<true>)
};
hipError_t launch_amvp_sad(const AmvpArgs& a, hipStream_t s);

// xMotionEstimation(bBi)'s search key (fme_mc.hip): the other list's uni-pred luma prediction at
// its MV (clipMv'd against the CU origin), key = 2 * org - pred (TComYuv::removeHighFreq), clipped
// to 8 bits with ClipForBiPredMe; w*h int16 at keys + key_off.  One task per wave.
struct BiKeyTask {
  uint16_t x, y;
  uint8_t w, h, org_id, ref_id;
  uint16_t cu_x, cu_y;
  int16_t mv_x, mv_y;
  int32_t key_off;
  uint32_t clip;
};
static_assert(sizeof(BiKeyTask) == 24, "BiKeyTask layout");
struct BiKeyArgs {
  const BiKeyTask* tasks;
  const PicDesc* pics;
  int16_t* keys;
  int32_t n;
  int32_t* invalid;           // device-resident requests: validated here, rejected ones counted
  int64_t n_keys;             // (then) the key buffer's length
  int32_t bit_depth;          // 8, or 10: uint16 planes, ClipForBiPredMe to 0..1023 (k_bi_key<true>)
};
hipError_t launch_bi_key(const BiKeyArgs& a, hipStream_t s);

// One prediction-error launch (fme_merge.hip k_pred_err): xGetInterPredictionError per task, the
// luma prediction of the task's motion and its SATD / SAD against the original.
struct PeArgs {
  const fme_pe_task* tasks;
  const PicDesc* pics;
  uint32_t* dist;             // per task; 0xFFFFFFFF for a skipped (invalid) one
  int32_t* invalid;           // count of skipped tasks
  int32_t n;
  int32_t bit_depth;          // 8, or 10: uint16 planes, the PU's sum >> 2
  int32_t use_hadamard;       // HADME (fme_config.use_hadamard)
};
hipError_t launch_pred_err(const PeArgs& a, hipStream_t s);

// One skip-check launch (fme_skip.hip k_pred_sse): the Y, Cb and Cr prediction of each task's
// motion and the three SSEs against the original (getDistPart with DF_SSE).
struct SseArgs {
  const fme_sse_task* tasks;
  const PicDesc* pics;
  uint32_t* sse;              // [n][3] Y, Cb, Cr; 0xFFFFFFFF x 3 for a skipped (invalid) task
  int32_t* invalid;           // count of skipped tasks
  int32_t n;
  int32_t bit_depth;          // 8, or 10: uint16 planes, each sample's square >> 4
};
hipError_t launch_pred_sse(const SseArgs& a, hipStream_t s);

// One cost-surface launch (fme_surface.hip k_cost_surface): the 49 quarter-pel distortions and costs
// around each job's integer MV (include/fme_surface.h).
struct SurfArgs {
  const fme_job* jobs;
  const uint8_t* probe;       // [n][2] position indices, or null: none
  fme_surface* surf;          // per job, or null; 0xFFFFFFFF in every word of an invalid job
  fme_surface_pick* pick;     // per job, or null
  const PicDesc* pics;
  const double* mlambda;      // [FME_MAX_LAMBDAS]
  const int16_t* keys;
  int64_t n_keys;
  int32_t* invalid;           // count of invalid jobs
  int32_t n;
  int32_t bit_depth;          // 8, or 10: uint16 planes, the PU's sum >> 2
  int32_t use_hadamard;       // HADME (fme_config.use_hadamard)
};
hipError_t launch_cost_surface(const SurfArgs& a, hipStream_t s);


// One batch as the device sees it.
struct BatchArgs {
  const fme_job* jobs;        // the batch as fme_job, or (packed entry points) null:
  const fme_job_packed* pjobs;   // the caller's packed rows, read in place (load_job)
  const int32_t* key_base;    // packed: key offset of each 64-job group's first keyed job, -1: none
  const int32_t* koff;        // packed: key offset per job, keyed jobs' entries only (k_classify writes them)
  fme_result* res;
  const int16_t* keys;
  int64_t n_keys;
  const double* mlambda;      // [FME_MAX_LAMBDAS]
  const PicDesc* pics;        // [FME_MAX_PICTURES]
  int32_t n;
  int32_t use_hadamard;
  int32_t fen;
  int32_t nn_mode;
  const int32_t* key_invalid; // > 0: the last device-built keys had invalid requests; batches
                              // whose jobs read keys are rejected (k_classify)
  const uint32_t* nn_in;      // NN input rows of FME_JOB_NN_IN jobs ([nn_in_cap][9]) or null
  int32_t nn_in_cap;
};

struct Schedule;

// Work buffers (device) for one batch.
struct WorkBufs {
  uint8_t* cls;          // [n] class id, 255 = invalid
  int32_t* perm;         // jobs grouped by class (original index): a refinement batch's class c at
                         // [c * perm_cap, + its count) (k_front); the integer search's classes densely in [0, n)
  int32_t* koff;         // [n] BatchArgs::koff as k_classify writes it (packed batches)
  int32_t* counts;       // [kNumClasses + 1]: per-class count, [24] = invalid jobs
  int32_t* counts_next;  // the other counter block: k_front's last workgroup zeroes it for the next batch
  int32_t* cursor;       // [kNumClasses]
  int32_t* blk_agg;      // [nblk * 9] per-block max of the NN writer indices
  int32_t* blk_prefix;   // [nblk * 9] exclusive prefix (carry-in) per block
  uint32_t* nn_state;    // 2 x 12 words: slot[8], c, pu_h, pu_w, written
  Schedule* sched;       // built on the device by k_front's last workgroup from the class totals
  int32_t* tile_ctr;     // [8] lane-kernel tile queue heads (part of the counter block)
  fme_mv_result* mv_out; // compact per-job output (fme_refine_mv*), or null
  int32_t perm_cap;      // jobs per class region of perm (the context's job capacity, >= n); the last
                         // member, so that the search kernels find the others where they were
};
// The search record of job i (the search writes its records in call order; the tail completes them).
__device__ __forceinline__ const fme_result* search_rec(const BatchArgs& a, const WorkBufs&, int i) { return a.res + i; }

// Schedule of the search kernel (k_front builds it on the device): class c's jobs are
// perm[class_off[c] .. + class_cnt[c]) and its 64-lane wave tiles [prefix[c], prefix[c+1]).
// class_off[c] = c * WorkBufs::perm_cap: the class regions do not depend on the counts, so a
// workgroup writes perm before the totals are known, and they are not adjacent.
struct Schedule {
  int32_t prefix[kNumClasses + 1];
  int32_t class_off[kNumClasses];
  int32_t class_cnt[kNumClasses];
  // The lane kernel's per-XCD tile queues.  Every class's wave tiles are split into 8 contiguous
  // bands (band x holds tiles [nt x / 8, nt (x+1) / 8) of a class with nt tiles), XCD x owns band x,
  // and its queue lists the band class by class in the order lane_class_at: xq[x][i] = the queue's
  // tiles before class lane_class_at(i); xq[x][kNumClasses] = its length.
  int32_t xq[8][kNumClasses + 1];
  int32_t invalid;            // jobs rejected by k_front (the whole batch is then skipped)
  int32_t pad_[3];
};
// The jobs of classes [c0, c1) in class order: how many there are, and where the q-th of them sits
// in perm (the kernels that walk several classes as one list: fme_px.hip).
__device__ __forceinline__ int sched_count(const Schedule* sc, int c0, int c1) {
  int n = 0;
  for (int c = c0; c < c1; c++) n += sc->class_cnt[c];
  return n;
}
__device__ __forceinline__ int sched_perm_index(const Schedule* sc, int c0, int c1, int q) {
  int c = c0;
  for (; c < c1 - 1 && q >= sc->class_cnt[c]; c++) q -= sc->class_cnt[c];
  return sc->class_off[c] + q;
}

// The two kernels of an NN-direct batch (fme_direct.hip, include/fme_direct.h) beside k_front and
// the tail: both walk the jobs in call order, 64 per workgroup, and do nothing in a batch k_front
// rejected (sched->invalid) except, in the evaluation, marking the compact records.
struct DirectArgs {
  BatchArgs a;                // a.res: the batch's records (the caller's, or the context's for the compact form)
  const Schedule* sched;      // of the batch's ring entry
  fme_mv_result* mv_out;      // the evaluation's compact output (fme_refine_direct_mv_device), or null
  int32_t n;
  int32_t bit_depth;          // 8, or 10: uint16 planes
};
// per job the EMI square step of fme_refine (or the FME_JOB_NN_IN row, or nothing): mv_int, c, emi[],
// n_emi into the record, every other field 0
hipError_t launch_direct_emi(const DirectArgs& d, hipStream_t s);
// per job the one sub-pel evaluation at the record's nn_class: mv, half / qtr, frac_cost, cost, bits
// and FME_RES_NN_DIRECT into the record (or the compact record)
hipError_t launch_direct_eval(const DirectArgs& d, hipStream_t s);

// The external predictor's two kernels (fme_extern.hip, include/fme_extern.h).
// What the evaluation reads beside a direct batch's arguments:
struct AtArgs {
  const fme_nn_row* rows;     // the jobs' NN input rows, or null: the EMI kernel wrote the records
  const uint8_t* cls;         // one class per job
  int32_t* refused;           // count of the jobs refused one by one (zeroed before the launch)
};
struct ExternArgs {
  DirectArgs d;               // d.a.res: the records (null with rows and the compact output)
  AtArgs at;
  int32_t n;
  int32_t bit_depth;
};
// per job the one sub-pel evaluation at at.cls[i]; the record's EMI fields from the row, or left as
// the EMI kernel wrote them
hipError_t launch_at_eval(const ExternArgs& x, hipStream_t s);
// the tail without the net: per job the NN inputs it resolves (a.res: the records the EMI kernel
// wrote) into rows[i], and the carried state from slot state_in to the other one, in every nn_mode;
// slot_reset: the loaded net's FME_NN_IN_SLOT_RESET rule
hipError_t launch_nn_rows(const BatchArgs& a, const WorkBufs& w, fme_nn_row* rows, int state_in, bool slot_reset,
                          hipStream_t s);

// Candidate-set refinement's two kernels (fme_among.hip, include/fme_among.h).
struct AmongArgs {
  DirectArgs d;               // d.a.res: the records (null with rows and the compact output)
  const fme_nn_row* rows;     // the jobs' NN input rows, or null: the EMI kernel wrote the records
  const uint8_t* cand;        // [n][k] candidate classes, FME_AMONG_EMPTY: an unused slot
  uint32_t* cand_cost;        // [n][k] the slots' costs, or null
  int32_t* refused;           // count of the jobs refused one by one (zeroed before the launch)
  int32_t k;                  // 1..FME_AMONG_MAX
  uint32_t status;            // the records' status bits
  int32_t row_status;         // 1: and the row's FME_RES_NN_STALE / _UNINIT (the top-K batch)
  int32_t n;
  int32_t bit_depth;
};
// per job the sub-pel evaluation at every class of its list and the record of the first least
hipError_t launch_among_eval(const AmongArgs& x, hipStream_t s);
// per row the k classes the two-layer net (nn_pack's layout) rates highest, best first
hipError_t launch_nn_rank(const fme_nn_row* rows, const float* nn_params, uint8_t* cand, int k, int n, hipStream_t s);

// What the schedule needs to know about the search kernel: lanes per PU of each class (its unit
// count rounded up to a power of two).
struct SchedParams {
  int32_t lanes[kNumClasses];
};
SchedParams sched_params();

// One integer-search launch (fme_tz.hip): the batch, its class order and the outputs.
struct TzArgs {
  BatchArgs a;
  const int32_t* perm;
  fme_job* jobs_out;          // mv_x / mv_y written per job
  const fme_tz_ext* ext;
  uint32_t* sad;              // may be null
  int16_t* emi_mv;            // [n][2] or null: the MV after the EMI square step (uni-pred EMI jobs)
  uint32_t* nn_in;            // [n][9] or null: FME_TZ_RING jobs' NN inputs (array_e[index_ref..+7], C)
  int32_t ext_stride;         // bytes per ext record: sizeof(fme_tz_ext), or sizeof(fme_tz_ext2) (predictors)
};
// Integer-search ext record i (either layout) and, for fme_tz_ext2 records, neighbour predictor k.
__device__ __forceinline__ fme_tz_ext tz_ext_at(const TzArgs& ta, int i) {
  return *reinterpret_cast<const fme_tz_ext*>(reinterpret_cast<const uint8_t*>(ta.ext) + (size_t)ta.ext_stride * i);
}
__device__ __forceinline__ void tz_pred_at(const TzArgs& ta, int i, int k, int& x, int& y) {
  if (ta.ext_stride < (int)sizeof(fme_tz_ext2)) {
    x = y = 0;
    return;
  }
  const fme_tz_ext2* e = reinterpret_cast<const fme_tz_ext2*>(reinterpret_cast<const uint8_t*>(ta.ext) + (size_t)ta.ext_stride * i);
  x = e->preds[k][0];
  y = e->preds[k][1];
}
// The bulk search's groups (fme_tz.hip k_tz_staged): PUs by (unit-shape kernel kid: 0 the 4x8
// units, 1 the 8x4, 2 the 8x8; reference picture; CTU), np = (bound picture ids) * cw * ch groups
// per kernel, at most kTzMaxPairs.
constexpr long long kTzMaxPairs = 1LL << 20;
struct TzPairs {
  int32_t* cnt;      // [3 np] PUs per group (zeroed before launch_tz_pairs)
  int32_t* cursor;   // [3 np]
  int32_t* off;      // [3 np] first position of each group in perm
  int32_t* seg;      // non-empty groups, kernel-major
  int32_t* nseg;     // [0..3): non-empty groups per kernel, [3..6): each kernel's first in seg
  int32_t* perm;     // [n] jobs grouped
  int32_t np, cw, ch;
};
hipError_t launch_tz_pairs(const TzArgs& ta, const TzPairs& tp, const uint8_t* cls, int n, hipStream_t s);
// keyed: some job of the batch reads a key block (bi-pred): the kernels that hold int16 keys;
// otherwise the uni-pred form, whose key rows take half the registers
hipError_t launch_tz_staged(const TzArgs& ta, const TzPairs& tp, int kid, bool keyed, int bit_depth, hipStream_t s);
// The dependency levels of a producer's m_integerMv2Nx2N chain (fme_tz.hip k_tz_level): jobs in
// level order, level l = jobs [lvl_off[l], lvl_off[l+1]), one launch per level, back to back.
struct TzChain {
  const int32_t* psrc;        // [n]: job whose post-EMI MV is m_integerMv2Nx2N, or -1
  int32_t nlev;
};
hipError_t launch_tz_levels(const TzArgs& ta, const TzChain& ch, const int32_t* h_lvl_off, int bit_depth, hipStream_t s);

// Host-side launch helpers (fme_kernels.hip).
// The picture / lambda tables as k_put_tables copies them from a pinned, device-mapped host slot
// (everything but a refinement batch).
struct TablesSlot {
  PicDesc pics[FME_MAX_PICTURES];
  double ml[FME_MAX_LAMBDAS];
};
// A refinement batch's tables as k_front's kernel argument: of each picture what the refinement
// kernels read, the luma plane (the chroma planes are motion compensation's and the skip check's,
// which read the shared device copy), so that the argument is 2 KB where the whole PicDesc table,
// 3.5 KB, would not fit the 4 KB argument segment beside the other arguments.
struct BatchPic {
  const uint8_t* luma;
  int32_t stride, width, height;
  int32_t pad_;
};
struct BatchTables {
  BatchPic pics[FME_MAX_PICTURES];
  double ml[FME_MAX_LAMBDAS];
};
// A refinement batch's front end in one pass: validation (against t), class, perm (class c at
// c * w.perm_cap), the NN writer maxima; its first workgroup writes t to d_pics / d_ml (what a.pics
// and a.mlambda name for the search and the tail; chroma fields null); the workgroup that finishes
// last writes *w.sched (block ranges, XCD queues, invalid count) and w.blk_prefix and zeroes
// w.counts_next
hipError_t launch_front(const BatchArgs& a, const WorkBufs& w, const SchedParams& p, const BatchTables& t,
                        PicDesc* d_pics, double* d_ml, hipStream_t s);
// The integer search's two passes (its class offsets are dense):
// validation, class and the class histogram in w.counts,
hipError_t launch_classify(const BatchArgs& a, const WorkBufs& w, hipStream_t s);
// then w.counts -> class offsets and the jobs grouped by class in perm[0, n) (block 0 also writes
// *w.sched with those offsets, which the integer search does not read, and zeroes w.counts_next)
hipError_t launch_scatter(const BatchArgs& a, const WorkBufs& w, const SchedParams& p, hipStream_t s);
// 12 words of NN state written to dst in stream order (reset / set_state)
hipError_t launch_put_state(uint32_t* dst, const uint32_t* v12, hipStream_t s);
// the picture / lambda tables written in stream order from a pinned, device-mapped host slot
hipError_t launch_put_tables(PicDesc* d_pics, double* d_ml, const TablesSlot* t_dev, hipStream_t s);
// The search kernel reads its schedule from *w.sched (no host round trip); it is launched with
// enough workgroups to fill the chip, each pulling tiles from its XCD's queue (then the other
// XCDs').  `a.n` bounds the work.
// reserve > 0: the grid is the resident workgroups (FME_LANE_WAVES per CU) less `reserve`
hipError_t launch_search_lane(const BatchArgs& a, const WorkBufs& w, int reserve, hipStream_t s);
// Bit depth 10 (main10): the pixel-per-lane search (fme_px.hip), same records as the lane kernel;
// pictures hold uint16 samples (PicDesc::luma reinterpreted, stride in samples).
// s_big (may be null: s): the stream of the large-PU kernel, run beside the small-PU one
hipError_t launch_search_px(const BatchArgs& a, const WorkBufs& w, int bit_depth, hipStream_t s, hipStream_t s_big);
// Bit depth 10: the lane-per-unit search on int16 samples (fme_lane10.hip), the lane kernel's
// classes, schedule and records (the default main10 search; FME_MAIN10_SEARCH=px selects the pixel
// kernel above)
hipError_t launch_search_lane10(const BatchArgs& a, const WorkBufs& w, hipStream_t s);
struct NnIn11 {   // NN_pred() inputs of a single call: array_e slots[8], C, PUHeight, PUWidth
  uint32_t v[11];
};
// The single-call server (fme_server.hip): its mailbox SrvBox, the request-block count and the
// payload mapping live in fme_srv_pack.h (shared with the host's packing code).  bit_depth selects
// the kernel instance (a context has one depth).
hipError_t launch_server(SrvBox* box, const float* nn, uint32_t served, uint32_t epoch, uint64_t idle_ticks,
                         uint64_t life_ticks, int bit_depth, hipStream_t s);
int lane_lanes_per_pu(int cls);                    // lanes of a class's PU group (pow2), 0: none
int lane_grid(int n, int reserve);                 // workgroups of a lane-kernel launch of n jobs (fme_lane.hip)
int cu_count(int device);                          // compute units (workgroup budget of a launch)
// Packed NN layout for the tail kernel (nn_pack, fme_kernels.hip): offsets in floats, every
// pair region 8-byte aligned.
constexpr int kNnPkPfx = 0;                       // [64 shapes][22] layer-1 prefix (k = 0..7)
constexpr int kNnPkW1 = kNnPkPfx + 64 * 22;       // [11 row pairs][9 k][2]   (k = 8..16)
constexpr int kNnPkW2 = kNnPkW1 + 11 * 9 * 2;     // [10][22][2]
constexpr int kNnPkW3 = kNnPkW2 + 10 * 22 * 2;    // [25][20][2] (row 49 zero)
constexpr int kNnPkB1 = kNnPkW3 + 25 * 20 * 2;    // 22
constexpr int kNnPkG1 = kNnPkB1 + 22;
constexpr int kNnPkBE1 = kNnPkG1 + 22;
constexpr int kNnPkB2 = kNnPkBE1 + 22;            // 20
constexpr int kNnPkG2 = kNnPkB2 + 20;
constexpr int kNnPkBE2 = kNnPkG2 + 20;
constexpr int kNnPkBout = kNnPkBE2 + 20;          // 50 (row 49 zero)
constexpr int kNnPkGin = kNnPkBout + 50;          // 9 each
constexpr int kNnPkMean = kNnPkGin + 9;
constexpr int kNnPkStd = kNnPkMean + 9;
constexpr int kNnPkFloats = kNnPkStd + 9 + 1;
static_assert(kNnPkW1 % 2 == 0 && kNnPkW2 % 2 == 0 && kNnPkW3 % 2 == 0 && kNnPkB1 % 2 == 0 &&
              kNnPkG1 % 2 == 0 && kNnPkBE1 % 2 == 0 && kNnPkB2 % 2 == 0 && kNnPkG2 % 2 == 0 &&
              kNnPkBE2 % 2 == 0 && kNnPkBout % 2 == 0, "pair regions must be 8-byte aligned");
void nn_pack(const float* params, float* packed);   // FME_NN_PARAMS floats -> kNnPkFloats
// NN_pred()'s embedding rows of PUHeight / PUWidth (the switches of TEncSearch.cpp:93-113)
__device__ __forceinline__ int emb_row_h(int h) {
  return h == 4 ? 1 : h == 8 ? 2 : h == 16 ? 3 : h == 12 ? 4 : h == 24 ? 5 : h == 32 ? 6 : h == 64 ? 7 : 0;
}
__device__ __forceinline__ int emb_row_w(int w) {
  return w == 4 ? 1 : w == 8 ? 2 : w == 12 ? 3 : w == 16 ? 4 : w == 24 ? 5 : w == 32 ? 6 : w == 64 ? 7 : 0;
}
typedef float f2 __attribute__((ext_vector_type(2)));   // a row pair of the packed layout
__device__ __forceinline__ f2 ld2(const float* __restrict__ Q, int o) { return *(const f2*)(Q + o); }
__device__ __forceinline__ f2 relu2(f2 s) {
  s.x = s.x < 0.0f ? 0.0f : s.x;
  s.y = s.y < 0.0f ? 0.0f : s.y;
  return s;
}
// Results download into pinned host memory (fme_download_device): `wgs` workgroups of 64 lanes.
hipError_t launch_download(const void* src, void* dst, size_t n16, int wgs, hipStream_t s);
// dst[q] = src[idx[q]] for q < n (jobs, and the integer-search extensions when both ext pointers are
// set): the producers' request order <-> dependency-level order on the device
hipError_t launch_gather_jobs(const fme_job* src, const fme_tz_ext* src_ext, const int32_t* idx, fme_job* dst,
                              fme_tz_ext* dst_ext, int n, hipStream_t s);
hipError_t launch_nn_tail(const BatchArgs& a, const WorkBufs& w, const float* nn_params,
                          int state_in, hipStream_t s);

// ---- the batch's jobs, either format -------------------------------------------------------------
// Global pointers typed as such (global_load, not flat); 16-byte rows at their 4-byte alignment.
typedef uint32_t job_u4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const job_u4 g_job_u4;
typedef __attribute__((address_space(1))) const uint32_t g_job_u32;
typedef __attribute__((address_space(1))) const int32_t g_job_i32;

// fme_job_packed row (pu, ctl, mv, mvp words) -> fme_job, as fme_unpack_jobs (fme_api.cpp) does:
// the range words are the canonical mv -/+ range bit, which gives the EMI step's four tests
// (xTZ8PointSquareSearch, TEncSearch.cpp:1341-1376) the packed answers.  key_offset: the job's key
// offset when its keyed bit is set (ignored otherwise).
__device__ __forceinline__ bool packed_keyed(uint32_t ctl) { return ((ctl >> 21) & 1u) != 0; }
__device__ __forceinline__ fme_job expand_job(job_u4 p, int32_t key_offset) {
  const uint32_t pu = p.x, ctl = p.y;
  const uint32_t rg = (ctl >> 22) & 15u;
  const int16_t mv_x = (int16_t)(p.z & 0xFFFFu), mv_y = (int16_t)(p.z >> 16);
  fme_job j;
  j.x = (uint16_t)((pu & 2047u) * 4u);
  j.y = (uint16_t)(((pu >> 11) & 2047u) * 4u);
  j.w = (uint8_t)((((pu >> 22) & 15u) + 1u) * 4u);
  j.h = (uint8_t)((((pu >> 26) & 15u) + 1u) * 4u);
  j.org_id = (uint8_t)(ctl & 63u);
  j.ref_id = (uint8_t)((ctl >> 6) & 63u);
  j.lambda_id = (uint8_t)((ctl >> 12) & 31u);
  j.flags = (uint8_t)((ctl >> 17) & 15u);
  j.bits_in = (uint16_t)(ctl >> 26);
  j.mv_x = mv_x;
  j.mv_y = mv_y;
  j.mvp_x = (int16_t)(p.w & 0xFFFFu);
  j.mvp_y = (int16_t)(p.w >> 16);
  j.lt_x = (int16_t)(mv_x - ((rg & FME_PK_RANGE_LEFT) ? 1 : 0));
  j.rb_x = (int16_t)(mv_x + ((rg & FME_PK_RANGE_RIGHT) ? 1 : 0));
  j.lt_y = (int16_t)(mv_y - ((rg & FME_PK_RANGE_TOP) ? 1 : 0));
  j.rb_y = (int16_t)(mv_y + ((rg & FME_PK_RANGE_BOTTOM) ? 1 : 0));
  j.key_offset = packed_keyed(ctl) ? key_offset : -1;
  return j;
}
__device__ __forceinline__ job_u4 packed_row(const BatchArgs& a, int i) { return *((g_job_u4*)a.pjobs + i); }

// Job i of the batch in registers: the caller's packed row expanded (one 16-byte load, and the key
// offset k_classify wrote for a keyed job), or the fme_job itself (two 16-byte loads).  Which of
// the two is a kernel argument, so the branch is wave-uniform.
__device__ __forceinline__ fme_job load_job(const BatchArgs& a, int i) {
  if (a.pjobs) {
    const job_u4 p = packed_row(a, i);
    int32_t ko = -1;
    if (packed_keyed(p.y)) ko = ((g_job_i32*)a.koff)[i];
    return expand_job(p, ko);
  }
  g_job_u4* const src = (g_job_u4*)(a.jobs + i);
  const job_u4 q0 = src[0], q1 = src[1];
  const uint32_t tmp[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  fme_job j;
  __builtin_memcpy(&j, tmp, sizeof(j));
  return j;
}
static_assert(sizeof(fme_job) == 32 && sizeof(fme_job_packed) == 16, "job layouts");
// PU size of job i alone (the tails' stale C / PU-size writer)
__device__ __forceinline__ void load_job_wh(const BatchArgs& a, int i, uint32_t& w, uint32_t& h) {
  if (a.pjobs) {
    const uint32_t pu = *(g_job_u32*)&a.pjobs[i].pu;
    w = (((pu >> 22) & 15u) + 1u) * 4u;
    h = (((pu >> 26) & 15u) + 1u) * 4u;
  } else {
    const uint32_t q = ((g_job_u32*)(a.jobs + i))[1];   // w, h, org_id, ref_id
    w = q & 0xFFu;
    h = (q >> 8) & 0xFFu;
  }
}

// The tail kernels' output: xMotionEstimation's MV / cost / bits with the NN class and status,
// into the full record or, for fme_refine_mv*, the compact one alone.
// The carried array_e slots a job writes (slots 0 .. n-1) and whether it writes C / PU size:
// FME_JOB_EMI: the EMI square step's pushes (its count by geometry, TEncSearch.cpp:1341-1376);
// FME_JOB_NN_IN: a whole input row (the backups' path: all 8 slots, unpushed ones 0, and C).
__device__ __forceinline__ int nn_pushes(const fme_job& j) {
  if (j.flags & FME_JOB_NN_IN) return 8;
  if (!(j.flags & FME_JOB_EMI)) return 0;
  const bool top = j.mv_y - 1 >= j.lt_y, bot = j.mv_y + 1 <= j.rb_y;
  const bool left = j.mv_x - 1 >= j.lt_x, right = j.mv_x + 1 <= j.rb_x;
  const int cols = 1 + (left ? 1 : 0) + (right ? 1 : 0);
  return (top ? cols : 0) + (left ? 1 : 0) + (right ? 1 : 0) + (bot ? cols : 0);
}
__device__ __forceinline__ bool nn_writes_c(const fme_job& j) { return (j.flags & (FME_JOB_EMI | FME_JOB_NN_IN)) != 0; }

// xMotionEstimation's tail (TEncSearch.cpp:4586-4597) for job j's quarter-pel MV (fx, fy), whose
// sub-pel cost is frac_cost: ruiBits = bits_in + the MV's bits, ruiCost = floor(fW (frac_cost -
// getCost(mvBits))) + getCost(ruiBits), fW 0.5 for a bi-pred iteration; double like
// TComRdCost::getCost, converted with gcc/x86-64's (Distortion)(double) semantics.  tail_job and the
// NN-direct evaluation (fme_direct.hip) call it.  (k_nn_deep_tail keeps its own statement of the
// same lines: through this function its load of frac_cost moves and its code changes.  For the same
// reason it keeps its own statement of the carried-input rule, which nn_carried below states for
// k_nn_tail and k_nn_rows: the deep tail is the one deliberate exception to both.)
__device__ __forceinline__ uint32_t me_tail(const fme_job& j, double ml, uint32_t frac_cost, int fx, int fy,
                                            uint32_t& bits) {
  const uint32_t mvb = simd::mv_bits(fx, fy, 0, j.mvp_x, j.mvp_y);
  bits = (uint32_t)j.bits_in + mvb;
  const double fw = (j.flags & FME_JOB_BIPRED) ? 0.5 : 1.0;
  const double val = floor(fw * ((double)frac_cost - (double)simd::mv_cost(ml, mvb))) + (double)simd::mv_cost(ml, bits);
  return (uint32_t)(int64_t)val;
}

// r: the job's record in call order (full-record output); src: its search record (the search
// writes its fields into r itself, so src == r and only the tail's fields are written here).
__device__ __forceinline__ void store_outputs(fme_result* r, const fme_result* src, fme_mv_result* mv_out, int i,
                                              int fx, int fy, uint32_t cost, uint32_t bits, uint8_t cls,
                                              uint16_t status) {
  if (mv_out) {
    fme_mv_result o;
    o.mv_x = (int16_t)fx;
    o.mv_y = (int16_t)fy;
    o.cost = cost;
    o.bits = bits;
    o.nn_class = cls;
    o.reserved = 0;
    o.status = status;
    mv_out[i] = o;
  } else {
    if (src != r) *r = *src;
    r->mv_x = (int16_t)fx;
    r->mv_y = (int16_t)fy;
    r->cost = cost;
    r->bits = bits;
    r->nn_class = cls;
    r->status = status;
  }
}

// Last-writer scan of NN_pred()'s carried globals, a workgroup at a time (k_nn_deep_tail; k_nn_tail
// uses writer_scan_wave below).  Job base + t of
// the block's NW waves (t = threadIdx.x) has run[f] = its index when it writes field f (array_e
// slot f < 8; f = 8: C and the PU size), else -1.  src[f] = the last writer at or before the job
// (carry[f]: the last writer before `base`, or -1); tot[f] = the block's last writer (or carry).
// Writer indices grow with the lane, so the last writer at or below a lane is the highest set bit
// of the wave's write mask at or below it: ballots and wave-uniform reads instead of a
// shuffle scan (each ds_bpermute step of which waited on the previous one).
template <int NW>
__device__ __forceinline__ void writer_scan(const int (&run)[9], const int (&carry)[9], int base,
                                            int32_t (*wave_tot)[9], int (&src)[9], int (&tot)[9]) {
  const int lane = (int)threadIdx.x & 63, wid = (int)threadIdx.x >> 6;
  const int wbase = base + 64 * wid;
  const unsigned long long below = ~0ull >> (63 - lane);
  int incl[9];
#pragma unroll
  for (int f = 0; f < 9; f++) {
    const unsigned long long mask = __ballot(run[f] >= 0);
    const unsigned long long m = mask & below;
    incl[f] = m ? wbase + 63 - __clzll(m) : -1;
    if (lane == 0) wave_tot[wid][f] = mask ? wbase + 63 - __clzll(mask) : -1;
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 9; f++) {
    const int t = lane < NW ? wave_tot[lane][f] : -1;
    const unsigned long long pm = __ballot(lane < wid && t >= 0);   // earlier waves with a writer
    const unsigned long long am = __ballot(t >= 0);
    const int prev = pm ? __builtin_amdgcn_readlane(t, 63 - __clzll(pm)) : carry[f];
    src[f] = max(incl[f], prev);
    tot[f] = am ? __builtin_amdgcn_readlane(t, 63 - __clzll(am)) : carry[f];
  }
}

// The same scan for a wave on its own (k_nn_tail): no LDS, no barrier, so the waves of a scan
// block need not run together.  The wave's first job is wbase; the writers of the earlier waves
// of its scan block are found by reading those jobs again, wave by wave backwards, until every
// field has one (usually the wave just before: most jobs push all eight slots) or the scan block's
// start, where carry[f] (k_scatter's blk_prefix) takes over.  `open` and the ballots are
// wave-uniform.
__device__ __forceinline__ void writer_scan_wave(const BatchArgs& a, const int (&run)[9], const int32_t* carry,
                                                 int wbase, int (&src)[9]) {
  const int lane = (int)threadIdx.x & 63;
  const unsigned long long below = ~0ull >> (63 - lane);
  int prev[9];
  unsigned open = 0x1FFu;   // fields whose last writer before wbase is not known yet
  for (int pb = wbase - 64; pb >= (wbase & ~(kJobsPerScanBlock - 1)) && open; pb -= 64) {
    const fme_job pj = load_job(a, pb + lane);   // pb + 63 < wbase < a.n
    const bool wr = nn_writes_c(pj);
    const int np = wr ? nn_pushes(pj) : 0;
#pragma unroll
    for (int f = 0; f < 9; f++) {
      const unsigned long long mask = __ballot(f < 8 ? np > f : wr);
      if ((open >> f & 1u) && mask) {
        prev[f] = pb + 63 - __clzll(mask);
        open &= ~(1u << f);
      }
    }
  }
#pragma unroll
  for (int f = 0; f < 9; f++) {
    if (open >> f & 1u) prev[f] = carry[f];
    const unsigned long long m = __ballot(run[f] >= 0) & below;
    src[f] = m ? wbase + 63 - __clzll(m) : prev[f];   // a writer in the wave is later than any before it
  }
}

// NN_pred()'s carried inputs as job i sees them: the one statement of the rule for k_nn_tail
// (tail_job) and k_nn_rows.  (k_nn_deep_tail is the deliberate exception and keeps its own: its
// invalid lanes run on through the net, and it reads the job's own pushes from memory.)
// Per carried field (array_e slot s < 8; field 8: C and the PU size), src[] being the last writer
// at or before the job (writer_scan_wave): the job's own push, from its record in registers
// (own_emi, own_c); else the record of the earlier writer; else the incoming state st_in.
// `written` is the state's mask with the fields some job of the batch wrote added.
// slot_reset (FME_NN_IN_SLOT_RESET, as in k_nn_deep_tail): the slots hold this job's own pushes and
// 0 elsewhere, and all count as written.
struct NnCarried {
  uint32_t e[8], c, ph, pw, written;
};
__device__ __forceinline__ void nn_carried(const BatchArgs& a, const WorkBufs& w, const uint32_t* st_in, int i,
                                           const fme_job& j, const int (&src)[9], const uint32_t (&own_emi)[8],
                                           uint32_t own_c, bool slot_reset, NnCarried& v) {
  v.written = st_in[11];
#pragma unroll
  for (int s = 0; s < 8; s++) {
    if (slot_reset) {
      v.e[s] = src[s] == i ? own_emi[s] : 0u;
      v.written |= 1u << s;
    } else if (src[s] == i) {
      v.e[s] = own_emi[s];
      v.written |= 1u << s;
    } else if (src[s] >= 0) {
      v.e[s] = search_rec(a, w, src[s])->emi[s];
      v.written |= 1u << s;
    } else {
      v.e[s] = st_in[s];
    }
  }
  if (src[8] == i) {
    v.c = own_c;
    v.ph = j.h;
    v.pw = j.w;
    v.written |= 0x100u;
  } else if (src[8] >= 0) {
    v.c = search_rec(a, w, src[8])->c;
    load_job_wh(a, src[8], v.pw, v.ph);
    v.written |= 0x100u;
  } else {
    v.c = st_in[8];
    v.ph = st_in[9];
    v.pw = st_in[10];
  }
}
// FME_RES_NN_STALE: the job did not push all of its own inputs; FME_RES_NN_UNINIT: a carried field
// that nothing has written yet, in this batch or before it.
__device__ __forceinline__ uint32_t nn_carried_status(bool writes_c, uint32_t own_n_emi, const NnCarried& v) {
  uint32_t status = 0;
  if (!writes_c || own_n_emi < 8) status |= FME_RES_NN_STALE;
  if ((v.written & 0x1FFu) != 0x1FFu) status |= FME_RES_NN_UNINIT;
  return status;
}
// The batch's last job carries what it saw to the next batch: the twelve state words.
__device__ __forceinline__ void nn_carry_on(uint32_t* st_out, const NnCarried& v) {
#pragma unroll
  for (int s = 0; s < 8; s++) st_out[s] = v.e[s];
  st_out[8] = v.c;
  st_out[9] = v.ph;
  st_out[10] = v.pw;
  st_out[11] = v.written;
}

// A batch k_classify rejected: every job is marked, nothing else is written, and the NN state
// is carried through unchanged (the host flips the state slot after every batch).
__device__ __forceinline__ void reject_job(const BatchArgs& a, const WorkBufs& w, int i, int state_in) {
  if (w.mv_out)
    w.mv_out[i].status = FME_RES_REJECTED;
  else
    a.res[i].status = FME_RES_REJECTED;
  if (i == 0)
    for (int k = 0; k < 12; k++) w.nn_state[12 * (state_in ^ 1) + k] = w.nn_state[12 * state_in + k];
}
}  // namespace fme
