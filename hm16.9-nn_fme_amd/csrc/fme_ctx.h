// fme_ctx.h — the host runtime's internal header: the context behind the C-ABI's opaque fme_ctx,
// its buffer types, the error helpers, and the few runtime functions (fme_api.cpp) that the
// predInterSearch producers (fme_producers.cpp) call.  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "fme_device.h"
#include "fme_overlap_host.h"

struct fme_ctx;

namespace fme {

// Records the text for fme_last_error (kept per thread, fme_api.cpp) and returns code.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                            \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      return fme::fail(_e == hipErrorOutOfMemory ? FME_E_NOMEM : FME_E_DEVICE, "%s: %s (%s:%d)", \
                       #expr, hipGetErrorString(_e), __FILE__, __LINE__);                        \
  } while (0)

// Passes a failed runtime call's FME_E_* code on (fail has recorded its text).
#define FME_TRY(expr)           \
  do {                          \
    const int _rc = (expr);     \
    if (_rc) return _rc;        \
  } while (0)

// Device memory (DevBuf) or pinned host memory (HostBuf: the producers' transfer buffers, full-rate
// DMA and no page faults on the buffers of the next call), grown on demand and freed with its owner.
template <typename T, bool kPinned>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept {
    std::swap(p, o.p), std::swap(cap, o.cap);
    return *this;
  }
  ~Buf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(kPinned ? n + n / 4 : n, 1);   // pinned: headroom, fewer regrowths
    void** const pp = reinterpret_cast<void**>(&p);
    hipError_t e = kPinned ? hipHostMalloc(pp, want * sizeof(T), hipHostMallocDefault) : hipMalloc(pp, want * sizeof(T));
    if (e == hipSuccess) cap = kPinned ? want : n;
    return e;
  }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using HostBuf = Buf<T, true>;

// An event / a stream that its holder created and destroys.  h is public and the handle converts
// implicitly, so hipEventCreate(&e.h), hipEventRecord(e, s) and `if (!e)` read as with a raw handle.
struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Event() {
    if (h) (void)hipEventDestroy(h);
  }
  operator hipEvent_t() const { return h; }
};
struct Stream {
  hipStream_t h = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : h(o.h) { o.h = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Stream() {
    if (h) (void)hipStreamDestroy(h);
  }
  operator hipStream_t() const { return h; }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<HostBuf<int>>::value &&
                  !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Stream>::value,
              "owners of device resources are move-only: a copy would free twice");

// The timing of a side launch (motion compensation, prediction error, SSE, cost surface, integer
// search): two events around the last launch made with profiling on (fme_api.cpp).
struct LaunchTimer {
  Event ev[2];
  bool timed = false;                        // the last launch was profiled
  int ensure(const fme_ctx* c);              // the events exist once profiling is on (begin calls it)
  int begin(const fme_ctx* c, hipStream_t s);   // before the launch
  int end(const fme_ctx* c, hipStream_t s);     // behind it
};
// The count of the tasks a side launch's kernel skipped: one device word, zeroed in stream order
// before the launch, and the stream of that launch.
struct InvalidCounter {
  DevBuf<int32_t> d;
  hipStream_t stream = nullptr;   // borrowed: the caller's stream of the last launch
  int zero(hipStream_t s);
};

// f(lo, hi) over [0, n) in up to 8 host threads (the producers' per-request loops; the caller's
// thread takes the first slice).
template <typename F>
void par_for(int n, F&& f) {
  const unsigned hc = std::thread::hardware_concurrency();
  const int nt = n < 32768 ? 1 : (int)std::min<unsigned>(8u, hc ? hc : 1u);
  if (nt <= 1) {
    f(0, n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve((size_t)nt - 1);
  for (int t = 1; t < nt; t++)
    th.emplace_back([&f, n, nt, t] { f((int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt)); });
  f(0, (int)((long long)n / nt));
  for (auto& x : th) x.join();
}
}  // namespace fme

// The deeper nets' single NN_pred call (k_nn_deep_single): class and completion word.
struct SingleStage {
  int32_t nn_out[4];
  uint32_t flag;                // completion word (call sequence number)
};

struct fme_ctx {
  int device = 0;
  fme_config cfg{};
  fme::PicDesc pics[FME_MAX_PICTURES]{};
  bool pic_owned[FME_MAX_PICTURES]{};
  size_t pic_bytes[FME_MAX_PICTURES]{};
  double mlambda[FME_MAX_LAMBDAS]{};
  bool lambda_set[FME_MAX_LAMBDAS]{};
  bool tables_dirty = true;

  // The device tables, 1 + kOvRing copies, copy t at d_pics.p + t * FME_MAX_PICTURES and
  // d_mlambda.p + t * FME_MAX_LAMBDAS.  Copy 0 is what everything but the refinement batches
  // reads (sync_tables: behind every batch in flight); copy 1 + r belongs to ring entry r
  // (fme_overlap_host.h) and is written by the k_front of every batch that has the entry, from
  // its kernel argument.  tab_gen counts the host tables' changes, shared_gen is the change copy 0
  // holds.
  fme::DevBuf<fme::PicDesc> d_pics;
  fme::DevBuf<double> d_mlambda;
  unsigned long long tab_gen = 1, shared_gen = 0;
  // copy 0's upload ring (sync_tables): pinned, device-mapped slots, each guarded by the event of
  // the launch that reads it
  static constexpr int kTabSlots = 16;
  fme::TablesSlot* h_tab = nullptr;
  fme::TablesSlot* h_tab_dev = nullptr;
  fme::Event tab_ev[kTabSlots];
  bool tab_used[kTabSlots] = {};
  int tab_next = 0;
  fme::DevBuf<int16_t> d_keys;
  size_t n_keys = 0;
  fme::DevBuf<float> d_nn;         // packed layout (nn_pack, kNnPkFloats)
  bool nn_loaded = false;
  // nn_mode 2: a generic net (fme_load_nn_net), packed by nn_deep_pack
  fme_nn_net net{};
  fme::DevBuf<uint8_t> d_net;
  bool net_loaded = false;
  int nn_engine = FME_NN_ENGINE_EXACT;
  float* nn_margin = nullptr;  // caller-owned device array (fme_set_nn_margin_output)
  int nn_margin_cap = 0;       // its length
  void* nn_logits = nullptr;   // caller-owned device array (fme_set_nn_logit_output), 49 per job
  int nn_logits_cap = 0;       // its length in jobs
  const uint32_t* nn_in = nullptr;   // caller-owned NN input rows of FME_JOB_NN_IN jobs (fme_set_nn_inputs)
  int nn_in_cap = 0;                 // its length in rows

  fme::DevBuf<fme_job> d_jobs;      // staging for fme_refine (host arrays)
  fme::DevBuf<fme_result> d_res;
  fme::DevBuf<fme_result> d_res1;    // the *_mv_* device entry points' records of a batch in slot 1
  fme::DevBuf<fme_mv_result> d_mv;   // staging for fme_refine_mv
  // What a batch's kernels hand each other (consecutive batches on two or three streams overlap:
  // fme_overlap_host.h); the integer search takes a batch number and with it a slot and a ring entry.
  // Per slot: what only the front end and the search touch.  Per ring entry: what the tail still reads.
  fme::DevBuf<uint8_t> cls[fme::kOvSlots];
  fme::DevBuf<int32_t> perm[fme::kOvSlots];
  fme::DevBuf<int32_t> koff[fme::kOvRing];    // packed batches: key offset per keyed job (k_front)
  fme::DevBuf<int32_t> blk_agg[fme::kOvRing];
  fme::DevBuf<int32_t> blk_prefix[fme::kOvRing];
  fme::DevBuf<int32_t> counts;      // kOvBlocks counter blocks (kCountWords each), used in rotation
  fme::OverlapState ov;             // batch count, the last three batches' streams, blocks in doubt
  // the batches' events: batch k records search_ev[k % kDoneRing] behind its search launch and
  // done_ev[k % kDoneRing] after its tail, each once
  static constexpr int kDoneRing = 16;
  fme::Event done_ev[kDoneRing];
  fme::Event search_ev[kDoneRing];
  // fme_nn_copy_state_device's reads of the carried state: the next batch's set / reset waits for the latest
  fme::Event state_read_ev[kDoneRing];
  long long state_reads = 0;
  hipEvent_t state_read_last = nullptr;      // borrowed: one of state_read_ev
  hipStream_t state_read_stream = nullptr;   // borrowed: the caller's
  int last_slot = 0;                // slot and ring entry of the last batch (fme_refine_status, fme_debug_front)
  int last_ring = 0;
  bool keys_fresh = false;          // the key buffer was written since the last batch
  fme::DevBuf<uint32_t> nn_state;   // 2 x 12 words
  int state_cur = 0;
  bool state_pending = false;   // reset / set_state not yet applied (next batch, stream order)
  uint32_t pending_state[12] = {};
  fme::DevBuf<fme::Schedule> d_sched;     // [kOvRing], built by k_front each batch
  fme::SchedParams sched_p{};
  int32_t* h_counts = nullptr; // pinned (freed by ~fme_ctx, like h_tab, stage and box)

  // motion compensation: owned chroma planes (cb then cr, one allocation per slot), staging
  uint8_t* chroma_owned[FME_MAX_PICTURES]{};
  size_t chroma_bytes[FME_MAX_PICTURES]{};
  fme::DevBuf<fme_mc_job> d_mc_jobs;
  fme::DevBuf<uint8_t> d_mc_planes;
  fme::InvalidCounter mc_invalid;
  // weighted prediction (fme_set_wp): [list][picture][Y, Cb, Cr], uploaded before a launch when changed
  fme_wp_param h_wp[2][FME_MAX_PICTURES][3] = {};
  bool wp_init = false, wp_dirty = true;
  fme::DevBuf<fme_wp_param> d_mc_wp;
  fme::LaunchTimer mc_timer;
  // prediction error / merge estimation (fme_merge.cpp): staging for the host entry points, the
  // skipped-task counter, the timer
  fme::DevBuf<fme_pe_task> d_pe_tasks;
  fme::DevBuf<uint32_t> d_pe_dist;
  fme::InvalidCounter pe_invalid;
  std::vector<fme_pe_task> h_pe_tasks;
  std::vector<uint32_t> h_pe_dist;
  fme::LaunchTimer pe_timer;
  // skip check (fme_skip.cpp): the same for the SSE launch
  fme::DevBuf<fme_sse_task> d_sse_tasks;
  fme::DevBuf<uint32_t> d_sse_out;       // [n][3]
  fme::InvalidCounter sse_invalid;
  std::vector<fme_sse_task> h_sse_tasks;
  std::vector<uint32_t> h_sse_out;
  fme::LaunchTimer sse_timer;
  // cost surface (fme_surface.cpp): staging for the host entry point, the invalid-job counter, the timer
  fme::DevBuf<fme_job> d_surf_jobs;
  fme::DevBuf<uint8_t> d_surf_probe;     // [n][2]
  fme::DevBuf<fme_surface> d_surf_out;
  fme::DevBuf<fme_surface_pick> d_surf_pick;
  fme::InvalidCounter surf_invalid;
  fme::LaunchTimer surf_timer;
  // NN-direct batches (include/fme_direct.h): timing events of the last one with profiling on: start,
  // front end, EMI, class and evaluation kernel ends
  fme::Event ev_direct[5];
  bool direct_timed = false;
  // the external predictor (include/fme_extern.h): staging of the host forms' rows and classes, the
  // count of the jobs the last fme_refine_at* batch refused one by one and that batch's end event (one
  // of done_ev), and the timing events of the last call of either family with profiling on: start,
  // front end, EMI, rows and evaluation kernel ends (extern_phases: bit 0 EMI, 1 rows, 2 evaluation ran)
  fme::DevBuf<fme_nn_row> d_ext_rows;
  fme::DevBuf<uint8_t> d_ext_cls;
  fme::DevBuf<int32_t> d_ext_refused;
  hipEvent_t ev_at_done = nullptr;   // borrowed: one of done_ev
  fme::Event ev_extern[5];
  unsigned extern_phases = 0;
  bool extern_timed = false;
  // candidate-set refinement (include/fme_among.h): the top-K batch's rows and candidates (sized for
  // max_jobs on first use), staging of the host forms' lists, rows and costs, the count of the jobs
  // the last among / top-K batch refused one by one and that batch's end event (one of done_ev), and
  // the timing events of the last call with profiling on: start, front end, EMI, rows, rank and
  // evaluation kernel ends (among_phases: bit 0 EMI, 1 rows, 2 rank, 3 evaluation ran)
  fme::DevBuf<fme_nn_row> d_am_rows;
  fme::DevBuf<uint8_t> d_am_cand;
  fme::DevBuf<uint32_t> d_am_cost;
  fme::DevBuf<int32_t> d_am_refused;
  hipEvent_t ev_among_done = nullptr;   // borrowed: one of done_ev
  fme::Event ev_among[6];
  unsigned among_phases = 0;
  bool among_timed = false;
  // integer search: staging for the host entry point, the timer
  fme::DevBuf<fme_tz_ext> d_tz_ext;
  fme::DevBuf<uint32_t> d_tz_sad;
  fme::DevBuf<uint32_t> d_tz_nn_in;   // staging of fme_integer_search_ring's NN input rows
  fme::LaunchTimer tz_timer;
  // phase wall times of the last producer call (fme_pred_inter_phases)
  double pi_ms[FME_PI_PHASES] = {};
  // predInterSearch producer: m_integerMv2Nx2N[REF_PIC_LIST_0][k] (TEncSearch.h:118), AMVP staging
  int16_t int_mv_2n[2][FME_MAX_REFS][2] = {};   // m_integerMv2Nx2N[list][ref]
  fme::DevBuf<fme::AmvpTask> d_amvp;
  fme::DevBuf<int16_t> d_tz_emi;   // [n][2] post-EMI integer MVs (producer levels)
  fme::DevBuf<uint32_t> d_amvp_sad;
  fme::DevBuf<fme::BiKeyTask> d_bikey;
  fme::DevBuf<int32_t> d_key_invalid;  // invalid requests of the last fme_build_bipred_keys_device
  fme::DevBuf<int32_t> d_ch_i32;     // k_tz_level: psrc
  fme::DevBuf<int32_t> d_tzp;        // staged integer search: 8 words (nseg), then cnt / cursor / off / seg (TzPairs)
  fme::DevBuf<int32_t> d_tzp_perm;   // [n] jobs grouped by (kernel, reference, CTU)
  // fme_pred_inter_p scratch, kept across calls: pinned transfer buffers, host arrays, the
  // level-ordered device copies of the jobs
  fme::HostBuf<fme::AmvpTask> h_pi_tasks;
  fme::HostBuf<uint32_t> h_pi_tsad;
  fme::HostBuf<fme_job> h_pi_jobs;
  fme::HostBuf<fme_tz_ext> h_pi_ext;
  fme::HostBuf<int32_t> h_pi_idx;      // [2 nj]: level order, then its inverse
  fme::HostBuf<int32_t> h_pi_psrc;
  fme::HostBuf<fme_mv_result> h_pi_mv;
  fme::HostBuf<fme_result> h_pi_last;  // the full records of the last 2Nx2N request
  fme::HostBuf<fme_result> h_pi_ures;  // fme_pred_inter_b: the uni-pred jobs' records
  fme::HostBuf<fme_job> h_pi_seq;      // fme_pred_inter_b: one round's jobs in call order
  fme::HostBuf<fme_mv_result> h_pi_rs; // fme_pred_inter_b: their results
  fme::HostBuf<uint32_t> h_pi_rows;    // fme_pred_inter_b: the bi jobs' NN input rows
  std::vector<int> pi_base, pi_task, pi_src, pi_lvl, pi_start, pi_byarea;
  std::vector<int32_t> pi_off, pi_fill;
  std::vector<uint8_t> pi_amvp_idx;
  fme::DevBuf<fme_job> d_pi_jobs;      // level order
  fme::DevBuf<fme_tz_ext> d_pi_ext;
  fme::DevBuf<int32_t> d_pi_idx;

  // The deeper nets' single NN_pred: inputs in the kernel argument, class and completion word in
  // pinned, device-mapped host memory.
  struct SingleStage* stage = nullptr;
  uint8_t* stage_dev = nullptr;
  fme::Stream single_stream;
  uint32_t single_seq = 0;
  // The single-call server (fme_server.hip) behind fme_frac_dif_single and the master net's
  // fme_nn_pred_single: its mailbox in pinned, device-mapped host memory, its own stream.
  fme::SrvBox* box = nullptr;
  fme::SrvBox* box_dev = nullptr;
  fme::Stream srv_stream;
  bool srv_running = false;
  bool srv_orphan = false;      // a wait on the instance timed out: it may still run on srv_stream
  // the streams this context's batches were issued on (note_stream): a buffer that a queued launch
  // may still read is regrown only after those streams have drained, not the whole device (borrowed:
  // the callers' streams and the context's own)
  static constexpr int kMaxStreams = 8;
  hipStream_t used_streams[kMaxStreams] = {};
  int n_used_streams = 0;
  bool used_overflow = false;   // more streams than tracked: fall back to a device synchronisation
  uint32_t srv_epoch = 0;       // of the instance launched last
  uint32_t srv_done = 0;        // sequence number of the last completed call
  uint32_t srv_nn_gen = 0;      // weight generation the running instance copied to LDS
  uint32_t nn_gen = 0;          // bumped by fme_load_nn_weights
  uint64_t srv_khz = 100000;    // wall-clock rate (s_memrealtime)
  bool srv_marks = false;       // the server records its phase checkpoints (fme_single_last_device_us)

  // Profiling: a ring of event sets, one per profiled batch, read once the batch has finished
  // (harvest_events), so profiling a run of batches adds no synchronisation.  Per set: 0 start,
  // 1 classify end = scatter begin, (2 unused,) 3 scatter end, 4 main search end, 5 search
  // end, 6 batch end.
  static constexpr int kEv = 9;
  static constexpr int kEvSets = 32;
  bool profiling = false;
  bool events_made = false;
  fme::Event ev[kEvSets][kEv];
  long long ev_head = 0;        // sets recorded
  long long ev_tail = 0;        // sets harvested
  bool timed = false;
  hipEvent_t ev_done = nullptr; // borrowed: end of the last batch, one of done_ev (fme_refine_status)
  hipEvent_t ev_search = nullptr; // borrowed: the caller's event, recorded before each search launch (fme_set_search_event)
  int search_reserve = 0;         // resident search workgroups left free (fme_set_search_reserve)
  bool main10_px = false;         // bit depth 10: the pixel kernel instead of the lane kernel
                                  // (environment FME_MAIN10_SEARCH=px, an A/B switch)
  bool batch_issued = false;
  float last_ms[FME_NUM_TIMINGS] = {};
  double acc_ms[FME_NUM_TIMINGS] = {};
  int acc_batches = 0;

  // auxiliary streams of the integer search (created on first use)
  fme::Stream aux, aux2;
  fme::Event ev_fork, ev_join, ev_join2;

  // What no member frees by itself: the owned picture planes and the pinned blocks.  Everything else
  // is a Buf, an Event or a Stream.  (fme_destroy has idled the device; fme_create's failure path
  // comes here with whatever it had reserved.)
  fme_ctx() = default;
  fme_ctx(const fme_ctx&) = delete;
  fme_ctx& operator=(const fme_ctx&) = delete;
  ~fme_ctx() {
    for (int i = 0; i < FME_MAX_PICTURES; i++) {
      if (pic_owned[i] && pics[i].luma) (void)hipFree(const_cast<uint8_t*>(pics[i].luma));
      if (chroma_owned[i]) (void)hipFree(chroma_owned[i]);
    }
    for (void* h : {(void*)h_counts, (void*)h_tab, (void*)stage, (void*)box})
      if (h) (void)hipHostFree(h);
  }
};

namespace fme {
size_t nn_deep_packed_bytes(const fme_nn_net& n);
void nn_deep_pack(const fme_nn_net& n, const double* params, void* out);
hipError_t launch_nn_deep_tail(const fme_nn_net& n, const void* packed, float* margin, void* logits, const BatchArgs& a,
                               const WorkBufs& w, int state_in, int engine, hipStream_t s);
hipError_t launch_nn_deep_single(const fme_nn_net& n, const void* packed, const NnIn11& in11, int32_t* out,
                                 uint32_t* flag, uint32_t seq, hipStream_t s);

// The runtime functions the producers call (fme_api.cpp, documented there).
// what every entry point but a refinement batch calls first: s waits for the refinement batches in
// flight on other streams, then slot 0's tables are brought up to date in stream order
int sync_tables(fme_ctx* c, hipStream_t s);
int grow_keys(fme_ctx* c, size_t n);   // called before the key buffer is written: the next batch serialises
BatchArgs batch_args(const fme_ctx* c, const fme_job* jobs, int n);   // the fields every batch shares
int refine_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, fme_mv_result* d_mv, int n, hipStream_t s,
                 const fme_job_packed* d_pjobs = nullptr, const int32_t* d_key_base = nullptr);
// an NN-direct batch (include/fme_direct.h): the front end, the EMI kernel, the tail as the class
// kernel, the evaluation kernel; planned like a batch that serialises (fme_overlap_host.h)
int direct_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, fme_mv_result* d_mv, int n, hipStream_t s);
int tz_run(fme_ctx* c, fme_job* d_jobs, const fme_tz_ext* d_ext, uint32_t* d_sad, int n, void* stream, int16_t* d_emi,
           uint32_t* d_nn_in = nullptr, int ext_stride = (int)sizeof(fme_tz_ext));
int check_rejected(fme_ctx* c, hipStream_t s, const char* name, const char* what);

// The readers of a side launch's timer and counter, by member: they check the context first.
// "<name>: null argument", "<name>: no profiled <what>"; the elapsed time of the last profiled launch
int timer_last_ms(fme_ctx* c, LaunchTimer fme_ctx::*timer, const char* name, const char* what, float* ms);
// "<name>: null ctx"; 0 before any launch; else waits (for the stream of the last launch, or with
// drain_all for every stream the context used) and returns the word
int invalid_count(fme_ctx* c, InvalidCounter fme_ctx::*counter, const char* name, bool drain_all = false);

// The host checks' form of the prediction kernels' task validators (mc_job_valid, pe_task_valid,
// sse_task_valid): PU shape, list flags, original picture, position, reference pictures.  The
// kind sets the flag mask, whether an original picture is named (motion compensation: width x
// height given), whether chroma planes are needed, and the texts.
enum PredKind { kPredMc, kPredErr, kPredSse };
const char* pred_task_problem(const fme_ctx* c, PredKind kind, int x, int y, int w, int h, unsigned flags,
                              const uint8_t* ref_id, unsigned org_id, int width, int height);
}  // namespace fme
