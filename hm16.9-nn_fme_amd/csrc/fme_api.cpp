// fme_api.cpp — host runtime behind the C-ABI of include/fme.h.
//
// A context owns one device's copies of the pictures, the motion-lambda table, the bi-pred key
// blocks, the NN weights, the NN_pred carried state (array_e slots, C, PUHeight, PUWidth,
// TEncSearch.cpp:55-57) and the per-batch work buffers.  A batch is
//   classify -> [one 100-byte D2H: class histogram] -> scatter -> search -> scan -> nn_tail
// on the caller's stream.  Errors are returned as FME_E_* codes; the text is kept per thread.
#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <memory>

#include "fme_among_host.h"
#include "fme_ctx.h"
#include "fme_direct_host.h"
#include "fme_extern_host.h"

using namespace fme;

namespace {
thread_local std::string g_last_error = "";
}  // namespace

// counts buffer: kOvBlocks counter blocks of kCountWords (fme_device.h: three 128-byte lines with the
// integer search's class histogram and k_front's done ticket, the 24 scatter cursors with k_front's
// invalid and keyed counts, and the 8 lane tile-queue heads), all zeroed at allocation.  Batch k
// counts in block k % kOvBlocks and its k_front (the workgroup that finishes last) zeroes the block
// of batch k + 2: no fill dispatch per batch, and no block is zeroed while the batch before or
// after, whose front end and search may run beside this one's on another stream, uses it
// (fme_overlap_host.h).  Whatever
// else touches the blocks (the integer search, a batch whose launches failed midway) leaves them
// in doubt (OverlapState::dirty), and the next batch starts, behind every batch in flight, with
// one hipMemsetAsync of all blocks.

int fme::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}


extern "C" {

int fme_abi_version(void) { return FME_ABI_VERSION; }

const char* fme_last_error(void) { return g_last_error.c_str(); }

int fme_create(int device, const fme_config* cfg, fme_ctx** out_ctx) {
  if (!cfg || !out_ctx) return fail(FME_E_INVALID, "fme_create: null argument");
  *out_ctx = nullptr;
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10)
    return fail(FME_E_UNSUPPORTED, "fme_create: bit_depth %d (8, or 10 for the main10 configurations)", cfg->bit_depth);
  if (cfg->nn_mode < 0 || cfg->nn_mode > 2) return fail(FME_E_INVALID, "fme_create: nn_mode %d", cfg->nn_mode);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(FME_E_INVALID, "fme_create: device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<fme_ctx> c(new fme_ctx());
  c->device = device;
  c->cfg = *cfg;
  HIP_TRY(c->d_pics.reserve((1 + kOvRing) * FME_MAX_PICTURES));
  HIP_TRY(c->d_mlambda.reserve((1 + kOvRing) * FME_MAX_LAMBDAS));
  HIP_TRY(c->d_nn.reserve(kNnPkFloats));
  HIP_TRY(c->counts.reserve(kOvBlocks * kCountWords));
  HIP_TRY(hipMemset(c->counts.p, 0, kOvBlocks * kCountWords * sizeof(int32_t)));
  HIP_TRY(c->d_sched.reserve(kOvRing));
  HIP_TRY(hipMemset(c->d_sched.p, 0, kOvRing * sizeof(Schedule)));
  for (auto& e : c->done_ev) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  for (auto& e : c->search_ev) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  c->sched_p = sched_params();
  {
    const char* m10 = std::getenv("FME_MAIN10_SEARCH");
    c->main10_px = m10 && std::strcmp(m10, "px") == 0;
  }
  HIP_TRY(c->nn_state.reserve(24));
  HIP_TRY(hipMemset(c->nn_state.p, 0, 24 * sizeof(uint32_t)));
  HIP_TRY(c->d_key_invalid.reserve(1));
  HIP_TRY(hipMemset(c->d_key_invalid.p, 0, sizeof(int32_t)));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_counts), kCountWords * sizeof(int32_t), hipHostMallocDefault));
  if (cfg->max_jobs > 0) {
    const size_t n = (size_t)cfg->max_jobs;
    const size_t nb = (n + kJobsPerScanBlock - 1) / kJobsPerScanBlock;
    if (n * kNumClasses > (size_t)INT32_MAX) return fail(FME_E_INVALID, "fme_create: max_jobs %d", cfg->max_jobs);
    for (int b = 0; b < kOvSlots; b++) {
      HIP_TRY(c->cls[b].reserve(n));
      HIP_TRY(c->perm[b].reserve(n * kNumClasses));   // one region of n jobs per class (k_front)
    }
    for (int r = 0; r < kOvRing; r++) {
      HIP_TRY(c->blk_agg[r].reserve(nb * 9));
      HIP_TRY(c->blk_prefix[r].reserve(nb * 9));
    }
  }
  *out_ctx = c.release();
  return FME_OK;
}

}  // extern "C"
static int srv_stop(fme_ctx* c);
// The end event of the batch `back` batches ago (1: the last one), or null; search_event: the
// event behind its search launch.
static hipEvent_t done_event(const fme_ctx* c, int back) {
  if (back < 1 || back > kOvBack || !c->ov.live[back - 1]) return nullptr;
  return c->done_ev[(c->ov.seq - back) % fme_ctx::kDoneRing];
}
static hipEvent_t search_event(const fme_ctx* c, int back) {
  if (back < 1 || back > kOvBack || !c->ov.live[back - 1]) return nullptr;
  return c->search_ev[(c->ov.seq - back) % fme_ctx::kDoneRing];
}
// s waits for the refinement batches in flight on other streams: at most three (the search of a
// batch waits for the end of the batch two before it, so the tail of batch k - 3 may be pending
// when batch k is planned).  A batch's end event fires after its search-end event, on the same
// stream: it covers both.
static int wait_batches(fme_ctx* c, hipStream_t s) {
  for (int back = 1; back <= kOvBack; back++)
    if (hipEvent_t e = done_event(c, back))
      if (c->ov.stream[back - 1] != s) HIP_TRY(hipStreamWaitEvent(s, e, 0));
  return FME_OK;
}
// Remember a stream this context issued work on (reads of its buffers may be queued there).
static void note_stream(fme_ctx* c, hipStream_t s) {
  for (int i = 0; i < c->n_used_streams; i++)
    if (c->used_streams[i] == s) return;
  if (c->n_used_streams < fme_ctx::kMaxStreams) c->used_streams[c->n_used_streams++] = s;
  else c->used_overflow = true;
}
// Wait for every launch of this context (its tracked streams; the device only if it used more),
// leaving other contexts' work alone.
static int drain_ctx(fme_ctx* c) {
  if (c->used_overflow) {
    HIP_TRY(hipDeviceSynchronize());
  } else {
    for (int i = 0; i < c->n_used_streams; i++) HIP_TRY(hipStreamSynchronize(c->used_streams[i]));
  }
  return FME_OK;
}
// Grows the bi-pred key buffer to n elements.  Growing frees the old buffer, which launches queued
// on the caller's stream, the integer search's auxiliary streams or another caller stream may still
// read: drain_ctx waits for the streams this context has used (for the whole device only when it
// used more than it tracks), and only when the buffer really grows.
int fme::grow_keys(fme_ctx* c, size_t n) {
  c->keys_fresh = true;   // its writer follows: the next batch waits for the batches in flight (one key buffer)
  if (n <= c->d_keys.cap) return FME_OK;
  FME_TRY(drain_ctx(c));   // no queued launch of this context still reads the old key buffer
  HIP_TRY(c->d_keys.reserve(n));
  return FME_OK;
}
extern "C" {
int fme_destroy(fme_ctx* c) {
  if (!c) return FME_OK;
  (void)hipSetDevice(c->device);
  (void)srv_stop(c);
  (void)hipDeviceSynchronize();
  delete c;
  return FME_OK;
}

// A new luma plane with other dimensions invalidates the slot's chroma planes.
static void keep_chroma(fme_ctx* c, int id, int width, int height) {
  const PicDesc& o = c->pics[id];
  if (o.luma && o.width == width && o.height == height) return;
  if (c->chroma_owned[id]) (void)hipFree(c->chroma_owned[id]);
  c->chroma_owned[id] = nullptr;
  c->chroma_bytes[id] = 0;
  c->pics[id].cb = c->pics[id].cr = nullptr;
  c->pics[id].cstride = 0;
}

int fme_set_picture(fme_ctx* c, int id, const uint8_t* luma, int stride, int width, int height, void* stream) {
  if (!c || !luma) return fail(FME_E_INVALID, "fme_set_picture: null argument");
  if (id < 0 || id >= FME_MAX_PICTURES) return fail(FME_E_INVALID, "fme_set_picture: id %d", id);
  if (width <= 0 || height <= 0 || stride < width || width > 65535 || height > 65535)
    return fail(FME_E_INVALID, "fme_set_picture: %dx%d stride %d", width, height, stride);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bps = c->cfg.bit_depth > 8 ? 2 : 1;   // bytes per sample (10-bit: uint16 samples)
  const size_t bytes = (size_t)width * height * bps;
  uint8_t* dst = c->pic_owned[id] ? const_cast<uint8_t*>(c->pics[id].luma) : nullptr;
  if (!dst || c->pic_bytes[id] < bytes) {
    if (dst) HIP_TRY(hipFree(dst));
    dst = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dst), bytes));
    c->pic_bytes[id] = bytes;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpy2DAsync(dst, width * bps, luma, stride * bps, width * bps, height, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // the caller may free its host plane on return
  keep_chroma(c, id, width, height);
  c->pics[id] = PicDesc{dst, width, width, height, c->pics[id].cb, c->pics[id].cr, c->pics[id].cstride, 0};
  c->pic_owned[id] = true;
  c->tables_dirty = true;
  return FME_OK;
}

int fme_bind_picture_device(fme_ctx* c, int id, const uint8_t* d_luma, int stride, int width, int height) {
  if (!c || !d_luma) return fail(FME_E_INVALID, "fme_bind_picture_device: null argument");
  if (id < 0 || id >= FME_MAX_PICTURES) return fail(FME_E_INVALID, "fme_bind_picture_device: id %d", id);
  if (width <= 0 || height <= 0 || stride < width) return fail(FME_E_INVALID, "fme_bind_picture_device: geometry");
  HIP_TRY(hipSetDevice(c->device));
  if (c->pic_owned[id] && c->pics[id].luma) HIP_TRY(hipFree(const_cast<uint8_t*>(c->pics[id].luma)));
  c->pic_owned[id] = false;
  c->pic_bytes[id] = 0;
  keep_chroma(c, id, width, height);
  c->pics[id] = PicDesc{d_luma, stride, width, height, c->pics[id].cb, c->pics[id].cr, c->pics[id].cstride, 0};
  c->tables_dirty = true;
  return FME_OK;
}

int fme_set_picture_chroma(fme_ctx* c, int id, const uint8_t* cb, const uint8_t* cr, int stride, void* stream) {
  if (!c || !cb || !cr) return fail(FME_E_INVALID, "fme_set_picture_chroma: null argument");
  if (id < 0 || id >= FME_MAX_PICTURES) return fail(FME_E_INVALID, "fme_set_picture_chroma: id %d", id);
  if (!c->pics[id].luma) return fail(FME_E_STATE, "fme_set_picture_chroma: picture %d has no luma plane", id);
  const int cw = c->pics[id].width >> 1, ch = c->pics[id].height >> 1;
  if (stride < cw) return fail(FME_E_INVALID, "fme_set_picture_chroma: stride %d < %d", stride, cw);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bps = c->cfg.bit_depth > 8 ? 2 : 1;   // bytes per sample (10-bit: uint16 planes)
  const size_t bytes = 2 * (size_t)cw * ch * bps;
  if (!c->chroma_owned[id] || c->chroma_bytes[id] < bytes) {
    if (c->chroma_owned[id]) HIP_TRY(hipFree(c->chroma_owned[id]));
    c->chroma_owned[id] = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->chroma_owned[id]), bytes));
    c->chroma_bytes[id] = bytes;
  }
  uint8_t* dcb = c->chroma_owned[id];
  uint8_t* dcr = dcb + (size_t)cw * ch * bps;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpy2DAsync(dcb, cw * bps, cb, stride * bps, cw * bps, ch, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpy2DAsync(dcr, cw * bps, cr, stride * bps, cw * bps, ch, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->pics[id].cb = dcb;
  c->pics[id].cr = dcr;
  c->pics[id].cstride = cw;
  c->tables_dirty = true;
  return FME_OK;
}

int fme_bind_picture_chroma_device(fme_ctx* c, int id, const uint8_t* d_cb, const uint8_t* d_cr, int stride) {
  if (!c || !d_cb || !d_cr) return fail(FME_E_INVALID, "fme_bind_picture_chroma_device: null argument");
  if (id < 0 || id >= FME_MAX_PICTURES) return fail(FME_E_INVALID, "fme_bind_picture_chroma_device: id %d", id);
  if (!c->pics[id].luma) return fail(FME_E_STATE, "fme_bind_picture_chroma_device: picture %d has no luma plane", id);
  if (stride < (c->pics[id].width >> 1)) return fail(FME_E_INVALID, "fme_bind_picture_chroma_device: stride %d", stride);
  HIP_TRY(hipSetDevice(c->device));
  if (c->chroma_owned[id]) HIP_TRY(hipFree(c->chroma_owned[id]));
  c->chroma_owned[id] = nullptr;
  c->chroma_bytes[id] = 0;
  c->pics[id].cb = d_cb;
  c->pics[id].cr = d_cr;
  c->pics[id].cstride = stride;
  c->tables_dirty = true;
  return FME_OK;
}

int fme_set_lambda(fme_ctx* c, int id, double lambda) {
  if (!c || id < 0 || id >= FME_MAX_LAMBDAS || !(lambda >= 0.0)) return fail(FME_E_INVALID, "fme_set_lambda: bad argument");
  // TComRdCost::setLambda: m_dLambdaMotionSAD[0] = 65536.0 * sqrt(lambda); selectMotionLambda
  // (true, 0, false) adds iAdd = 0 (TComRdCost.cpp:104-110, TComRdCost.h:159).
  const double sq = std::sqrt(lambda);
  c->mlambda[id] = 65536.0 * sq + 0;
  c->lambda_set[id] = true;
  c->tables_dirty = true;
  return FME_OK;
}

int fme_set_motion_lambda(fme_ctx* c, int id, double ml) {
  if (!c || id < 0 || id >= FME_MAX_LAMBDAS || !(ml >= 0.0)) return fail(FME_E_INVALID, "fme_set_motion_lambda: bad argument");
  c->mlambda[id] = ml;
  c->lambda_set[id] = true;
  c->tables_dirty = true;
  return FME_OK;
}

int fme_set_keys(fme_ctx* c, const int16_t* keys, size_t count, void* stream) {
  if (!c || (!keys && count)) return fail(FME_E_INVALID, "fme_set_keys: null argument");
  HIP_TRY(hipSetDevice(c->device));
  // the upload and the memset below are GPU work: a resident single-call server could hold them up
  // on a hardware queue its stream shares (sync_tables does the same for batches)
  FME_TRY(srv_stop(c));
  FME_TRY(grow_keys(c, count));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FME_TRY(wait_batches(c, s));   // a batch in flight on another stream may still read the keys
  if (count) HIP_TRY(hipMemcpyAsync(c->d_keys.p, keys, count * sizeof(int16_t), hipMemcpyHostToDevice, s));
  // fresh host keys: a rejection left by an earlier device build no longer applies (fme.h: rejected
  // "until keys are built again"), in stream order with the upload
  HIP_TRY(hipMemsetAsync(c->d_key_invalid.p, 0, sizeof(int32_t), s));
  HIP_TRY(hipStreamSynchronize(s));
  c->n_keys = count;
  return FME_OK;
}

int fme_load_nn_weights(fme_ctx* c, const float* params, int count) {
  if (!c || !params) return fail(FME_E_INVALID, "fme_load_nn_weights: null argument");
  if (count != FME_NN_PARAMS) return fail(FME_E_INVALID, "fme_load_nn_weights: %d params, expected %d", count, FME_NN_PARAMS);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<float> packed(kNnPkFloats);
  nn_pack(params, packed.data());
  HIP_TRY(hipMemcpy(c->d_nn.p, packed.data(), kNnPkFloats * sizeof(float), hipMemcpyHostToDevice));
  c->nn_loaded = true;
  c->nn_gen++;   // a running server instance holds the old weights in LDS: it is restarted
  return FME_OK;
}

int fme_nn_param_count(const fme_nn_net* n) {
  if (!n) return fail(FME_E_INVALID, "fme_nn_param_count: null descriptor");
  if (n->n_hidden < 1 || n->n_hidden > FME_NN_MAX_HIDDEN)
    return fail(FME_E_INVALID, "fme_nn_param_count: n_hidden %d", n->n_hidden);
  if (n->precision != FME_NN_F32 && n->precision != FME_NN_F64)
    return fail(FME_E_INVALID, "fme_nn_param_count: precision %d", n->precision);
  if (n->embedding < FME_NN_EMB_NONE || n->embedding > FME_NN_EMB_SWAP)
    return fail(FME_E_INVALID, "fme_nn_param_count: embedding %d", n->embedding);
  if (n->out_act != FME_NN_OUT_LINEAR && n->out_act != FME_NN_OUT_SIGMOID)
    return fail(FME_E_INVALID, "fme_nn_param_count: out_act %d", n->out_act);
  if (n->carry_hidden >> n->n_hidden) return fail(FME_E_INVALID, "fme_nn_param_count: carry_hidden 0x%x", n->carry_hidden);
  if (n->input_flags & ~(FME_NN_IN_SLOT_RESET | FME_NN_IN_TZ_RING))
    return fail(FME_E_INVALID, "fme_nn_param_count: input_flags 0x%x", n->input_flags);
  if ((n->input_flags & FME_NN_IN_TZ_RING) && ((n->input_flags & FME_NN_IN_SLOT_RESET) || n->carry_hidden))
    return fail(FME_E_INVALID, "fme_nn_param_count: FME_NN_IN_TZ_RING with FME_NN_IN_SLOT_RESET or carry_hidden");
  int count = n->embedding ? 64 : 0, fan = n->embedding ? 17 : 9;
  for (int l = 0; l < n->n_hidden; l++) {
    const int w = n->width[l];
    if (w < 1 || w > FME_NN_MAX_WIDTH) return fail(FME_E_INVALID, "fme_nn_param_count: width[%d] = %d", l, w);
    count += w * fan + 3 * w;
    fan = w;
  }
  return count + 49 * fan + 49 + 27;
}

int fme_load_nn_net(fme_ctx* c, const fme_nn_net* n, const double* params, int count) {
  if (!c || !n || !params) return fail(FME_E_INVALID, "fme_load_nn_net: null argument");
  const int need = fme_nn_param_count(n);
  if (need < 0) return need;
  if (count != need) return fail(FME_E_INVALID, "fme_load_nn_net: %d params, the descriptor needs %d", count, need);
  if (n->carry_hidden)
    return fail(FME_E_UNSUPPORTED, "fme_load_nn_net: carry_hidden 0x%x (hidden layers carried across calls) is not "
                "supported by the batch engines", n->carry_hidden);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = nn_deep_packed_bytes(*n);
  if (!bytes) return fail(FME_E_UNSUPPORTED, "fme_load_nn_net: no kernel for this net");
  std::vector<unsigned char> packed(bytes);
  nn_deep_pack(*n, params, packed.data());
  FME_TRY(drain_ctx(c));   // a batch of this context in flight may still read the previous net
  HIP_TRY(c->d_net.reserve(bytes));
  HIP_TRY(hipMemcpy(c->d_net.p, packed.data(), bytes, hipMemcpyHostToDevice));
  c->net = *n;
  c->net_loaded = true;
  return FME_OK;
}

int fme_set_nn_engine(fme_ctx* c, int engine) {
  if (!c || (engine != FME_NN_ENGINE_EXACT && engine != FME_NN_ENGINE_MFMA))
    return fail(FME_E_INVALID, "fme_set_nn_engine: bad argument");
  c->nn_engine = engine;
  return FME_OK;
}

int fme_set_nn_logit_output(fme_ctx* c, void* d_logits, int capacity) {
  if (!c) return fail(FME_E_INVALID, "fme_set_nn_logit_output: null ctx");
  if (d_logits && capacity <= 0) return fail(FME_E_INVALID, "fme_set_nn_logit_output: capacity %d", capacity);
  c->nn_logits = capacity > 0 ? d_logits : nullptr;
  c->nn_logits_cap = d_logits ? capacity : 0;
  return FME_OK;
}

int fme_set_nn_inputs(fme_ctx* c, const uint32_t* d_rows, int capacity) {
  if (!c) return fail(FME_E_INVALID, "fme_set_nn_inputs: null ctx");
  if (d_rows && capacity <= 0) return fail(FME_E_INVALID, "fme_set_nn_inputs: capacity %d", capacity);
  c->nn_in = capacity > 0 ? d_rows : nullptr;
  c->nn_in_cap = d_rows ? capacity : 0;
  return FME_OK;
}

int fme_set_nn_margin_output(fme_ctx* c, float* d_margin, int capacity) {
  if (!c) return fail(FME_E_INVALID, "fme_set_nn_margin_output: null ctx");
  if (d_margin && capacity <= 0) return fail(FME_E_INVALID, "fme_set_nn_margin_output: capacity %d", capacity);
  c->nn_margin = capacity > 0 ? d_margin : nullptr;
  c->nn_margin_cap = d_margin ? capacity : 0;
  return FME_OK;
}

int fme_nn_reset_state(fme_ctx* c) {
  if (!c) return fail(FME_E_INVALID, "fme_nn_reset_state: null ctx");
  for (uint32_t& v : c->pending_state) v = 0;
  c->state_pending = true;
  return FME_OK;
}

int fme_nn_get_state(fme_ctx* c, uint32_t* out12) {
  if (!c || !out12) return fail(FME_E_INVALID, "fme_nn_get_state: null argument");
  if (c->state_pending) {
    std::memcpy(out12, c->pending_state, sizeof(c->pending_state));
    return FME_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  FME_TRY(drain_ctx(c));   // this context's streams only
  HIP_TRY(hipMemcpy(out12, c->nn_state.p + 12 * c->state_cur, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FME_OK;
}

int fme_nn_set_state(fme_ctx* c, const uint32_t* in12) {
  if (!c || !in12) return fail(FME_E_INVALID, "fme_nn_set_state: null argument");
  std::memcpy(c->pending_state, in12, sizeof(c->pending_state));
  c->state_pending = true;
  return FME_OK;
}

int fme_nn_copy_state_device(fme_ctx* c, uint32_t* d_out12, void* stream) {
  if (!c || !d_out12) return fail(FME_E_INVALID, "fme_nn_copy_state_device: null argument");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (c->state_pending) {
    HIP_TRY(launch_put_state(d_out12, c->pending_state, s));
    return FME_OK;
  }
  // The copy reads the words the last batch's tail wrote: s waits for that batch where it ran on
  // another stream.  The next batch may set or reset those words before its tail, on another
  // stream again, so it waits for this read first (hand_state_on): an event per copy, from a ring,
  // recorded once per use; only the latest is ever waited for.
  FME_TRY(wait_batches(c, s));
  HIP_TRY(hipMemcpyAsync(d_out12, c->nn_state.p + 12 * c->state_cur, 12 * sizeof(uint32_t),
                         hipMemcpyDeviceToDevice, s));
  Event& e = c->state_read_ev[c->state_reads++ % fme_ctx::kDoneRing];
  if (!e) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(e, s));
  c->state_read_last = e;
  c->state_read_stream = s;
  return FME_OK;
}

}  // extern "C"

// perm holds one region per PU class, each as long as the context's job capacity (k_front writes
// class c's jobs from c * capacity on, whatever the batch's class totals turn out to be): 96 bytes
// per job of capacity, 83 MB for a 1080p frame's 862,920 jobs; and that once per batch slot.
// The ring entries (fme_overlap_host.h) hold what the tail still reads: koff, 4 bytes per job of
// capacity, and the scan blocks' 72 bytes per 1,024 jobs; 3.5 MB per entry for that frame.
// All slots and entries are sized together.  *grows (may be null): a buffer had to grow (freeing
// the old one waits for the device, so no batch in flight loses a buffer it reads).
static int ensure_work(fme_ctx* c, int n, bool* grows = nullptr) {
  const size_t nb = ((size_t)n + kJobsPerScanBlock - 1) / kJobsPerScanBlock;
  if ((size_t)n * kNumClasses > (size_t)INT32_MAX) return fail(FME_E_INVALID, "%d jobs in one batch", n);
  if (grows) *grows = (size_t)n > c->cls[0].cap || (size_t)n > c->koff[0].cap;
  for (int b = 0; b < kOvSlots; b++) {
    HIP_TRY(c->cls[b].reserve(n));
    HIP_TRY(c->perm[b].reserve((size_t)n * kNumClasses));
  }
  for (int r = 0; r < kOvRing; r++) {
    HIP_TRY(c->blk_agg[r].reserve(nb * 9));
    HIP_TRY(c->blk_prefix[r].reserve(nb * 9));
    HIP_TRY(c->koff[r].reserve(n));
  }
  return FME_OK;
}

// The work buffers of a planned batch: its slot's perm and cls, its ring entry's koff, scan blocks
// and Schedule, counting in its counter block; the front end's last workgroup zeroes the block
// the plan names.
static WorkBufs work_bufs(fme_ctx* c, const OverlapPlan& plan) {
  WorkBufs w{};
  w.cls = c->cls[plan.slot].p;
  w.perm = c->perm[plan.slot].p;
  w.perm_cap = (int32_t)(c->perm[plan.slot].cap / kNumClasses);
  w.koff = c->koff[plan.ring].p;
  w.counts = c->counts.p + plan.block * kCountWords;
  w.counts_next = c->counts.p + plan.block_zeroed * kCountWords;
  w.cursor = w.counts + kCursorWord;
  w.tile_ctr = w.counts + kTileCtrWord;
  w.blk_agg = c->blk_agg[plan.ring].p;
  w.blk_prefix = c->blk_prefix[plan.ring].p;
  w.nn_state = c->nn_state.p;
  w.sched = c->d_sched.p + plan.ring;
  w.mv_out = nullptr;
  return w;
}

BatchArgs fme::batch_args(const fme_ctx* c, const fme_job* jobs, int n) {
  BatchArgs a{};
  a.jobs = jobs;
  a.keys = c->d_keys.p;
  a.n_keys = (int64_t)c->n_keys;
  a.key_invalid = c->d_key_invalid.p;
  a.mlambda = c->d_mlambda.p;
  a.pics = c->d_pics.p;
  a.n = n;
  a.use_hadamard = c->cfg.use_hadamard ? 1 : 0;
  a.fen = c->cfg.fast_inter_mode;
  return a;
}

// What every batch entry point does with its stream before it enqueues anything.
static int enter_stream(fme_ctx* c, hipStream_t s) {
  note_stream(c, s);
  // a resident server could hold up this work on a hardware queue its stream shares: stop it
  // (a few microseconds; the next single call relaunches it)
  return srv_stop(c);
}

// The picture / lambda tables go to the device in stream order, never through a copy engine:
// rebinding pictures for the next frame never waits for the batch in flight, and the batch stream
// holds no copy-engine transfer (which would queue behind bulk uploads).  A refinement batch
// carries them in k_front's kernel argument, and k_front writes the batch's ring entry's copy
// (batch_begin).  Everything else reads copy 0, which a one-block kernel brings up to date here
// when the host tables changed since its last upload; its readers are over before this launch
// (sync_tables waits for the batches in flight, and those read their ring entries' copies).
static int put_tables(fme_ctx* c, hipStream_t s) {
  FME_TRY(enter_stream(c, s));
  if (c->tables_dirty) {
    c->tab_gen++;
    c->tables_dirty = false;
  }
  if (c->shared_gen == c->tab_gen) return FME_OK;
  if (!c->h_tab) {
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, fme_ctx::kTabSlots * sizeof(TablesSlot), hipHostMallocMapped));
    c->h_tab = static_cast<TablesSlot*>(p);
    void* d = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&d, p, 0));
    c->h_tab_dev = static_cast<TablesSlot*>(d);
    for (auto& e : c->tab_ev) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  }
  const int k = c->tab_next;
  c->tab_next = (k + 1) % fme_ctx::kTabSlots;
  if (c->tab_used[k]) HIP_TRY(hipEventSynchronize(c->tab_ev[k]));   // its last launch has run
  std::memcpy(c->h_tab[k].pics, c->pics, sizeof(c->pics));
  std::memcpy(c->h_tab[k].ml, c->mlambda, sizeof(c->mlambda));
  HIP_TRY(launch_put_tables(c->d_pics.p, c->d_mlambda.p, c->h_tab_dev + k, s));
  HIP_TRY(hipEventRecord(c->tab_ev[k], s));
  c->tab_used[k] = true;
  c->shared_gen = c->tab_gen;
  return FME_OK;
}

int fme::sync_tables(fme_ctx* c, hipStream_t s) {
  FME_TRY(wait_batches(c, s));
  return put_tables(c, s);
}

// ---- what the side launches share (fme_ctx.h) ----------------------------------------------------
int LaunchTimer::ensure(const fme_ctx* c) {
  if (c->profiling)
    for (auto& e : ev)
      if (!e) HIP_TRY(hipEventCreate(&e.h));
  return FME_OK;
}
int LaunchTimer::begin(const fme_ctx* c, hipStream_t s) {
  FME_TRY(ensure(c));
  if (c->profiling) HIP_TRY(hipEventRecord(ev[0], s));
  return FME_OK;
}
int LaunchTimer::end(const fme_ctx* c, hipStream_t s) {
  if (c->profiling) HIP_TRY(hipEventRecord(ev[1], s));
  timed = c->profiling;
  return FME_OK;
}
int fme::timer_last_ms(fme_ctx* c, LaunchTimer fme_ctx::*timer, const char* name, const char* what, float* ms) {
  if (!c || !ms) return fail(FME_E_INVALID, "%s: null argument", name);
  const LaunchTimer& t = c->*timer;
  if (!t.timed) return fail(FME_E_STATE, "%s: no profiled %s", name, what);
  HIP_TRY(hipEventSynchronize(t.ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, t.ev[0], t.ev[1]));
  return FME_OK;
}

int InvalidCounter::zero(hipStream_t s) {
  HIP_TRY(d.reserve(1));
  HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(int32_t), s));
  stream = s;
  return FME_OK;
}
int fme::invalid_count(fme_ctx* c, InvalidCounter fme_ctx::*counter, const char* name, bool drain_all) {
  if (!c) return fail(FME_E_INVALID, "%s: null ctx", name);
  const InvalidCounter& k = c->*counter;
  if (!k.d.p) return 0;
  HIP_TRY(hipSetDevice(c->device));
  int32_t v = 0;
  if (drain_all) FME_TRY(drain_ctx(c));
  else HIP_TRY(hipStreamSynchronize(k.stream));
  HIP_TRY(hipMemcpy(&v, k.d.p, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

const char* fme::pred_task_problem(const fme_ctx* c, PredKind kind, int x, int y, int w, int h, unsigned flags,
                                   const uint8_t* ref_id, unsigned org_id, int width, int height) {
  const bool mc = kind == kPredMc, sse = kind == kPredSse;
  if (w < 4 || h < 4 || w > 64 || h > 64 || (w & 3) || (h & 3)) return sse ? "block size" : "PU size";
  const unsigned lists = FME_MC_L0 | FME_MC_L1, more = mc ? FME_MC_WP : sse ? 0u : FME_PE_LOSSLESS;
  if (!(flags & lists) || (flags & ~(lists | more))) return "list flags";
  if (!mc) {   // the picture is the original's
    if (org_id >= FME_MAX_PICTURES || !c->pics[org_id].luma) return "original picture";
    const PicDesc& o = c->pics[org_id];
    if (sse && (!o.cb || !o.cr)) return "original picture without chroma planes";
    width = o.width;
    height = o.height;
  }
  if (x + w > width || y + h > height) return sse ? "block outside the picture" : "PU outside the picture";
  for (int l = 0; l < 2; l++) {
    if (!(flags & (1u << l))) continue;
    if (ref_id[l] >= FME_MAX_PICTURES) return mc ? "reference id" : "reference picture";
    const PicDesc& p = c->pics[ref_id[l]];
    if (mc && (!p.luma || !p.cb || !p.cr)) return "reference picture without luma + chroma";
    if (!p.luma) return "reference picture";
    if (sse && (!p.cb || !p.cr)) return "reference picture without chroma planes";
    if (p.width != width || p.height != height) return "reference picture dimensions";
  }
  return nullptr;
}


// Applies a reset / set of the NN state requested since the last batch, in stream order (before the
// batch's tail, once the stream has waited for the previous batch's tail: that tail writes the
// words this sets).
static int apply_pending_state(fme_ctx* c, hipStream_t s) {
  if (!c->state_pending) return FME_OK;
  HIP_TRY(launch_put_state(c->nn_state.p + 12 * c->state_cur, c->pending_state, s));
  c->state_pending = false;
  return FME_OK;
}

// Profiling: a ring of event sets; a set is read once its batch has finished (polled at the next
// batch, waited for only when the ring is full or the caller asks for the timings).
static int harvest_events(fme_ctx* c, bool wait_all) {
  while (c->ev_tail != c->ev_head) {
    const int b = c->ev_tail % fme_ctx::kEvSets;
    const Event* e = c->ev[b];
    if (wait_all) {
      HIP_TRY(hipEventSynchronize(e[6]));
    } else {
      const hipError_t q = hipEventQuery(e[6]);
      if (q == hipErrorNotReady) break;
      HIP_TRY(q);
    }
    float* ms = c->last_ms;
    HIP_TRY(hipEventElapsedTime(&ms[0], e[0], e[3]));   // k_front: classify, scatter and schedule in one pass
    ms[1] = 0.f;                                        // (the scatter's own launch, until k_front)
    HIP_TRY(hipEventElapsedTime(&ms[2], e[3], e[5]));
    HIP_TRY(hipEventElapsedTime(&ms[3], e[5], e[6]));
    HIP_TRY(hipEventElapsedTime(&ms[4], e[0], e[6]));
    HIP_TRY(hipEventElapsedTime(&ms[5], e[3], e[4]));
    ms[6] = 0.f;   // no auxiliary search kernel any more (every shape runs in the lane kernel)
    for (int i = 0; i < FME_NUM_TIMINGS; i++) c->acc_ms[i] += ms[i];
    c->acc_batches++;
    c->timed = true;
    c->ev_tail++;
  }
  return FME_OK;
}

// ---- the batch scaffold -------------------------------------------------------------------------
// A context enqueues four kinds of batch: the ordinary one (refine_batch), the NN-direct one
// (direct_batch, include/fme_direct.h) and the external predictor's two (inputs_batch and at_batch,
// include/fme_extern.h).  They are one scaffold with different middles, all enqueued without waiting
// for the device:
//   batch_begin    the plan and its waits, the tables, the arguments, k_front
//   the kind's own launches and event records, with hand_state_on before whatever writes the NN state
//   batch_end      the end event and the bookkeeping that every reader of a finished batch relies on
// Only the ordinary batch overlaps its neighbours.  The other three are planned with kOvForeign: a
// batch number of their own, so that slot, ring entry and counter block are nobody else's and
// k_front leaves the block after next zeroed, but serial: they start behind every batch in flight
// (batch_open's waits are sync_tables' wait_batches), the batch after them starts behind their end
// event, and the front end of the batch after that waits for it too, so nothing runs beside them.
// The integer search (tz_run) has a front end of its own and shares the inner pieces alone:
// batch_open and batch_close.
namespace {
struct Batch {
  uint32_t features;   // the kOv* word it is planned and committed with
  OverlapPlan plan;    // fme_overlap_host.h: its slot, ring entry and counter block, and what its stream waits for
  hipEvent_t search_end, done;
  BatchArgs a;
  WorkBufs w;
};
}  // namespace

// What a planned batch (or integer search) does before its first launch: the plan, its two events,
// the waits of the plan that come before the front end, the fill of the counter blocks when they
// are in doubt, and its work buffers.  Nothing on the device waits for another batch: every
// dependency is a stream wait on an earlier batch's event.
static int batch_open(fme_ctx* c, hipStream_t s, uint32_t features, Batch* b) {
  b->features = features;
  b->plan = overlap_plan(c->ov, s, features);
  const OverlapPlan& plan = b->plan;
  // this batch's events: recorded once per use; before an entry of a ring is recorded again, the
  // waits queued on its last record (by the three batches after that one) have been passed, which
  // the end of the last of the three says
  b->search_end = c->search_ev[c->ov.seq % fme_ctx::kDoneRing];
  b->done = c->done_ev[c->ov.seq % fme_ctx::kDoneRing];
  if (c->ov.seq >= fme_ctx::kDoneRing)
    HIP_TRY(hipEventSynchronize(c->done_ev[(c->ov.seq + kOvBack) % fme_ctx::kDoneRing]));
  if (plan.serial) {   // behind every batch in flight
    if (plan.wait_prev_front) HIP_TRY(hipStreamWaitEvent(s, done_event(c, 1), 0));
    if (plan.wait_slot) HIP_TRY(hipStreamWaitEvent(s, done_event(c, 2), 0));
    if (plan.wait_back3) HIP_TRY(hipStreamWaitEvent(s, done_event(c, 3), 0));
  } else if (plan.wait_front) {
    // search k - 2 is over: perm and cls of the slot and its counter block are free; the tail of
    // batch k - 2 may be pending, it reads its own ring entry
    HIP_TRY(hipStreamWaitEvent(s, search_event(c, 2), 0));
  } else if (plan.wait_front_end) {
    HIP_TRY(hipStreamWaitEvent(s, done_event(c, 2), 0));   // batch k - 2 was serialised: all of it
  }
  // The counter block is zero: batch k - 2's k_front left it so (the first batches' blocks
  // fme_create zeroed).  After a batch that was abandoned on the host half-way all blocks are
  // filled here.  Its launches carry no end event, so the host waits for the context's streams
  // first (an error path); the batch after this one waits for this one's end (kOvFill), so it does
  // not start under the fill.
  if (plan.fill_blocks) {
    FME_TRY(drain_ctx(c));
    HIP_TRY(hipMemsetAsync(c->counts.p, 0, kOvBlocks * kCountWords * sizeof(int32_t), s));
  }
  b->w = work_bufs(c, plan);
  return FME_OK;
}

// Every launch is enqueued: the end event, and the plan is committed (the counter blocks are out of
// doubt again; a batch that returns before this leaves them to the next batch's fill).
static int batch_close(fme_ctx* c, hipStream_t s, const Batch& b) {
  HIP_TRY(hipEventRecord(b.done, s));
  overlap_commit(c->ov, s, b.features, b.plan);
  return FME_OK;
}

// Everything up to and including k_front.  The jobs are fme_job rows, or (d_jobs null) the
// fme_job_packed rows d_pjobs with d_key_base, read in place by every kernel.  extra: the kind's own
// feature bits; nn_mode: what the kernels see; zero (may be null): a counter zeroed behind the
// batch's waits, before its first launch (its last user, an earlier batch, is over); ev_start /
// ev_front (null when not profiling): recorded before and behind k_front.
// a.nn_in is the context's binding in every kind: the external predictor's entry points refuse to
// run while rows are bound (extern_enter), so theirs is null with capacity 0.
static int batch_begin(fme_ctx* c, const fme_job* d_jobs, const fme_job_packed* d_pjobs, const int32_t* d_key_base,
                       fme_result* d_res, int n, hipStream_t s, uint32_t extra, int nn_mode, int32_t* zero,
                       hipEvent_t ev_start, hipEvent_t ev_front, Batch* b) {
  bool grows = false;
  FME_TRY(ensure_work(c, n, &grows));
  const uint32_t features = extra | (c->keys_fresh ? kOvKeys : 0u) |
                            (d_jobs && d_jobs == c->d_jobs.p ? kOvStaged : 0u) | (grows ? kOvGrow : 0u);
  FME_TRY(enter_stream(c, s));   // (touches nothing the plan reads)
  FME_TRY(batch_open(c, s, features, b));
  if (zero) HIP_TRY(hipMemsetAsync(zero, 0, sizeof(int32_t), s));
  // The batch's picture / lambda tables travel in k_front's kernel argument; k_front validates
  // against them and writes them to the ring entry's device copy, which the later kernels read.
  PicDesc* const d_pics = c->d_pics.p + (1 + b->plan.ring) * FME_MAX_PICTURES;
  double* const d_ml = c->d_mlambda.p + (1 + b->plan.ring) * FME_MAX_LAMBDAS;
  BatchTables tab;
  for (int i = 0; i < FME_MAX_PICTURES; i++)
    tab.pics[i] = BatchPic{c->pics[i].luma, c->pics[i].stride, c->pics[i].width, c->pics[i].height, 0};
  std::memcpy(tab.ml, c->mlambda, sizeof(c->mlambda));
  BatchArgs& a = b->a;
  a = batch_args(c, d_jobs, n);
  a.pics = d_pics;
  a.mlambda = d_ml;
  a.pjobs = d_jobs ? nullptr : d_pjobs;
  a.key_base = d_key_base;
  a.koff = c->koff[b->plan.ring].p;
  a.res = d_res;
  a.nn_mode = nn_mode;
  a.nn_in = c->nn_in;
  a.nn_in_cap = c->nn_in_cap;
  if (ev_start) HIP_TRY(hipEventRecord(ev_start, s));
  // the counter block is zero (batch_open); the blocks stay in doubt until every launch of the
  // batch is enqueued (batch_close)
  overlap_begin(c->ov);
  HIP_TRY(launch_front(a, b->w, c->sched_p, tab, d_pics, d_ml, s));
  if (ev_front) HIP_TRY(hipEventRecord(ev_front, s));
  return FME_OK;
}

// Before whatever writes the NN state (a tail, k_nn_rows).  The writers hand the state on: this one
// runs after the previous batch's, the one dependency between consecutive batches, and a reset /
// set of the state belongs between the two.  Only an overlapping batch has wait_prev_tail: a serial
// plan has waited for batch k - 1 before anything (overlap_plan: wait_prev_front = serial && other1,
// wait_prev_tail = other1 && !wait_prev_front, so serial implies !wait_prev_tail), and kOvForeign
// makes a plan serial; the three serial kinds enqueue no wait here.
static int hand_state_on(fme_ctx* c, hipStream_t s, const Batch& b) {
  if (b.plan.wait_prev_tail) HIP_TRY(hipStreamWaitEvent(s, done_event(c, 1), 0));
  if (c->state_read_last) {   // a copy of the state the previous writer left (fme_nn_copy_state_device) comes first
    if (c->state_read_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->state_read_last, 0));
    c->state_read_last = nullptr;
  }
  return apply_pending_state(c, s);
}

// The end event and what a finished batch leaves: ev_done, last_slot / last_ring
// (fme_refine_status), keys_fresh, batch_issued, the committed plan and, where the batch wrote the
// other NN state slot (advanced), state_cur (fme_nn_get_state, fme_nn_copy_state_device).
static int batch_end(fme_ctx* c, hipStream_t s, const Batch& b, bool advanced) {
  FME_TRY(batch_close(c, s, b));
  c->ev_done = b.done;
  c->last_slot = b.plan.slot;
  c->last_ring = b.plan.ring;
  c->keys_fresh = false;
  c->batch_issued = true;
  if (advanced) c->state_cur ^= 1;
  return FME_OK;
}

// The NN of a batch that runs one is loaded, and the caller's margin / logit outputs hold n jobs.
static int nn_ready(const fme_ctx* c, int n, const char* name, const char* family) {
  if (c->cfg.nn_mode == 1 && !c->nn_loaded) return fail(FME_E_STATE, "%s: nn_mode set but no weights loaded", name);
  if (c->cfg.nn_mode == 2 && !c->net_loaded) return fail(FME_E_STATE, "%s: nn_mode 2 but no net loaded", name);
  if (c->cfg.nn_mode == 2 && c->nn_margin && n > c->nn_margin_cap)
    return fail(FME_E_INVALID, "%s: %d jobs but the margin output holds %d", family, n, c->nn_margin_cap);
  if (c->cfg.nn_mode == 2 && c->nn_logits && n > c->nn_logits_cap)
    return fail(FME_E_INVALID, "%s: %d jobs but the logit output holds %d", family, n, c->nn_logits_cap);
  return FME_OK;
}

// The NN + xMotionEstimation tail of the context's nn_mode, on the batch's stream.
// (Where it becomes runnable after the next batch's search has started, that search's persistent
// workgroups hold every wave slot and the tail runs as they drain; on a stream of the highest
// priority it did the same, since resident workgroups are not displaced: DESIGN.md section 5 "Batch
// overlap".  The front end of batch k + 2 does not wait for it: it reads this batch's ring entry,
// the front end writes another.)
static hipError_t launch_tail(const fme_ctx* c, const Batch& b, hipStream_t s) {
  return c->cfg.nn_mode == 2
             ? launch_nn_deep_tail(c->net, c->d_net.p, c->nn_margin, c->nn_logits, b.a, b.w, c->state_cur, c->nn_engine, s)
             : launch_nn_tail(b.a, b.w, c->d_nn.p, c->state_cur, s);
}

// The EMI and evaluation kernels' arguments (fme_direct.hip, fme_extern.hip).
static DirectArgs direct_args(const fme_ctx* c, const Batch& b) {
  DirectArgs da{};
  da.a = b.a;
  da.sched = b.w.sched;
  da.n = b.a.n;
  da.bit_depth = c->cfg.bit_depth;
  return da;
}

// The ordinary batch: k_front -> search -> NN + tail.
// Device validation covers what the host cannot see for device-resident jobs: a job with an
// unknown PU shape, an unset picture / lambda slot or a key block outside the key buffer makes
// k_front mark the batch rejected; every later kernel then skips its work.
// d_jobs null: the batch is d_pjobs / d_key_base (fme_job_packed rows).
int fme::refine_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, fme_mv_result* d_mv, int n,
                      hipStream_t s, const fme_job_packed* d_pjobs, const int32_t* d_key_base) {
  FME_TRY(nn_ready(c, n, "fme_refine_device", "fme_refine"));
  HIP_TRY(hipSetDevice(c->device));
  const bool prof = c->profiling;
  const Event* ev = nullptr;
  if (prof) {
    FME_TRY(harvest_events(c, false));
    if (c->ev_head - c->ev_tail == fme_ctx::kEvSets) {   // ring full: wait for the oldest set
      HIP_TRY(hipEventSynchronize(c->ev[c->ev_tail % fme_ctx::kEvSets][6]));
      FME_TRY(harvest_events(c, false));
    }
    ev = c->ev[c->ev_head % fme_ctx::kEvSets];
  }
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, d_pjobs, d_key_base, d_res, n, s,
                      (c->cfg.nn_mode == 2 ? kOvDeepNn : 0u) | (c->cfg.bit_depth > 8 && c->main10_px ? kOvPx : 0u),
                      c->cfg.nn_mode ? 1 : 0, nullptr, prof ? ev[0] : nullptr, prof ? ev[3] : nullptr, &b));
  b.w.mv_out = d_mv;   // (k_front writes no records)
  // the search writes the slot's internal records, which the tail of batch k - 2 reads
  if (b.plan.wait_search) HIP_TRY(hipStreamWaitEvent(s, done_event(c, 2), 0));
  if (c->ev_search) HIP_TRY(hipEventRecord(c->ev_search, s));
  // the lane kernels: every PU shape, one launch on the batch stream, 8-bit (fme_lane.hip) or
  // 10-bit (fme_lane10.hip); with FME_MAIN10_SEARCH=px the pixel kernels at bit depth 10 (fme_px.hip)
  if (c->cfg.bit_depth > 8) {
    // the small- and large-PU pixel kernels one after the other: side by side on two streams they
    // took 11.5 ms per 1080p frame against 10.5 in series (profiles/r06_ab.log: their LDS and
    // wave slots compete)
    if (c->main10_px)
      HIP_TRY(launch_search_px(b.a, b.w, c->cfg.bit_depth, s, nullptr));
    else
      HIP_TRY(launch_search_lane10(b.a, b.w, s));
  } else {
    HIP_TRY(launch_search_lane(b.a, b.w, c->search_reserve, s));
  }
  if (prof) HIP_TRY(hipEventRecord(ev[4], s));
  HIP_TRY(hipEventRecord(b.search_end, s));   // what the front end of batch k + 2 waits for
  FME_TRY(hand_state_on(c, s, b));
  if (prof) HIP_TRY(hipEventRecord(ev[5], s));
  HIP_TRY(launch_tail(c, b, s));
  if (prof) {
    HIP_TRY(hipEventRecord(ev[6], s));
    c->ev_head++;
  }
  return batch_end(c, s, b, b.a.nn_mode != 0);
}

// After a refinement batch: the rejected-job count comes down, one synchronisation, FME_E_INVALID if any.
int fme::check_rejected(fme_ctx* c, hipStream_t s, const char* name, const char* what) {
  HIP_TRY(hipMemcpyAsync(c->h_counts, &c->d_sched.p[c->last_ring].invalid, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c->h_counts[0] > 0)
    return fail(FME_E_INVALID, "%s: %d job(s) %s", name, c->h_counts[0], what);
  return FME_OK;
}

// Host arrays: H2D of the jobs into the context's staging buffer, the batch (run), D2H of its
// output (d_out, in a buffer the caller reserved) and of the rejected-job count, one
// synchronisation at the end.
template <class Run>
static int host_batch(fme_ctx* c, const fme_job* jobs, int n, hipStream_t s, const char* name, void* out,
                      const void* d_out, size_t out_bytes, Run run) {
  HIP_TRY(c->d_jobs.reserve(n));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  FME_TRY(run());
  HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
  return check_rejected(c, s, name, "with an unsupported PU size or unset picture/lambda/key");
}

// The *_mv_* device entry points' full records (the search writes them, the tail reads them): context
// scratch, one buffer per batch slot (the next batch's slot: the batch follows at once and plans
// the same batch number).  The host-array entry points and the producers pass c->d_res whichever
// slot their batch has: they are serialised before and after (kOvStaged), so no batch beside them
// uses it.
static int slot_records(fme_ctx* c, int n, fme_result** out) {
  DevBuf<fme_result>& b = c->ov.seq % kOvSlots ? c->d_res1 : c->d_res;
  HIP_TRY(b.reserve(n));
  *out = b.p;
  return FME_OK;
}

// The NN-direct batch (include/fme_direct.h): k_front -> EMI kernel -> NN tail -> evaluation kernel.
// The class kernel is the ordinary tail, launched as it is on the records the EMI kernel wrote,
// whose frac_cost is a placeholder (0): what the tail derives from it (cost, bits) and its mv are
// overwritten by the evaluation kernel, which follows in stream order, so no reader sees them: the
// caller's records are complete only behind the evaluation kernel, and the compact form's tail
// writes the context's internal records, never the caller's array (mv_out stays null for it).
int fme::direct_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, fme_mv_result* d_mv, int n,
                      hipStream_t s) {
  FME_TRY(nn_ready(c, n, "fme_refine_direct", "fme_refine_direct"));
  const bool prof = c->profiling;
  Event* ev = c->ev_direct;
  if (prof)
    for (int k = 0; k < 5; k++)
      if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k].h));
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, nullptr, nullptr, d_res, n, s, kOvForeign | (c->cfg.nn_mode == 2 ? kOvDeepNn : 0u), 1,
                      nullptr, prof ? ev[0] : nullptr, prof ? ev[1] : nullptr, &b));
  DirectArgs da = direct_args(c, b);
  HIP_TRY(launch_direct_emi(da, s));
  if (prof) HIP_TRY(hipEventRecord(ev[2], s));
  HIP_TRY(hipEventRecord(b.search_end, s));
  FME_TRY(hand_state_on(c, s, b));
  HIP_TRY(launch_tail(c, b, s));
  if (prof) HIP_TRY(hipEventRecord(ev[3], s));
  da.mv_out = d_mv;
  HIP_TRY(launch_direct_eval(da, s));
  if (prof) HIP_TRY(hipEventRecord(ev[4], s));
  c->direct_timed = prof;
  return batch_end(c, s, b, true);
}

// The direct entry points' common start: the argument check (fme_direct_host.h); *run: enqueue.
static int direct_enter(fme_ctx* c, const void* jobs, const void* out, int n, const char* name, bool* run) {
  *run = false;
  const int rq = direct_request(c, jobs, out, n, c ? c->cfg.nn_mode : 1);
  if (rq == FME_E_STATE) return fail(rq, "%s: nn_mode 0 has no class to evaluate", name);
  if (rq < 0) return fail(rq, "%s: bad argument (n = %d)", name, n);
  if (rq == 0) {
    HIP_TRY(hipSetDevice(c->device));
    *run = true;
  }
  return FME_OK;
}

// ---- the external predictor (include/fme_extern.h) -----------------------------------------------
// Both batches are a direct batch cut at the class.  Their profiling events: [0] / [1] around
// k_front, [2] behind the EMI kernel, [3] behind the rows kernel, [4] behind the evaluation.
static int extern_events(fme_ctx* c) {
  if (c->profiling)
    for (auto& e : c->ev_extern)
      if (!e) HIP_TRY(hipEventCreate(&e.h));
  c->extern_timed = false;   // until the batch is enqueued in full
  return FME_OK;
}

// The inputs batch: k_front -> EMI kernel (on d_rec, context-internal records) -> rows kernel.  It
// hands the NN state on like a tail, in every nn_mode: it writes the other state slot.
static int inputs_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_rec, fme_nn_row* d_rows, int n, hipStream_t s) {
  const bool prof = c->profiling;
  const Event* ev = c->ev_extern;
  FME_TRY(extern_events(c));
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, nullptr, nullptr, d_rec, n, s, kOvForeign, 1, nullptr, prof ? ev[0] : nullptr,
                      prof ? ev[1] : nullptr, &b));
  HIP_TRY(launch_direct_emi(direct_args(c, b), s));
  if (prof) HIP_TRY(hipEventRecord(ev[2], s));
  HIP_TRY(hipEventRecord(b.search_end, s));
  FME_TRY(hand_state_on(c, s, b));
  const bool slot_reset = c->cfg.nn_mode == 2 && c->net_loaded && (c->net.input_flags & FME_NN_IN_SLOT_RESET);
  HIP_TRY(launch_nn_rows(b.a, b.w, d_rows, c->state_cur, slot_reset, s));
  if (prof) HIP_TRY(hipEventRecord(ev[3], s));
  c->extern_phases = 3u;
  c->extern_timed = prof;
  return batch_end(c, s, b, true);
}

// The evaluation batch: k_front -> EMI kernel unless the caller brought rows -> evaluation at the
// caller's classes.  d_res: the full records (with d_mv and no rows: context-internal ones the EMI
// kernel writes; with d_mv and rows: null).  The NN state is not touched.
static int at_batch(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cls,
                    fme_result* d_res, fme_mv_result* d_mv, int n, hipStream_t s) {
  HIP_TRY(c->d_ext_refused.reserve(1));
  const bool prof = c->profiling;
  const Event* ev = c->ev_extern;
  FME_TRY(extern_events(c));
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, nullptr, nullptr, d_res, n, s, kOvForeign, 1, c->d_ext_refused.p,
                      prof ? ev[0] : nullptr, prof ? ev[1] : nullptr, &b));
  ExternArgs x{};
  x.d = direct_args(c, b);
  if (!d_rows) {
    HIP_TRY(launch_direct_emi(x.d, s));
    if (prof) HIP_TRY(hipEventRecord(ev[2], s));
  }
  HIP_TRY(hipEventRecord(b.search_end, s));
  x.d.mv_out = d_mv;
  x.at = AtArgs{d_rows, d_cls, c->d_ext_refused.p};
  x.n = n;
  x.bit_depth = c->cfg.bit_depth;
  HIP_TRY(launch_at_eval(x, s));
  if (prof) HIP_TRY(hipEventRecord(ev[4], s));
  c->extern_phases = d_rows ? 4u : 5u;
  c->extern_timed = prof;
  FME_TRY(batch_end(c, s, b, false));
  c->ev_at_done = b.done;
  return FME_OK;
}


// The families' common start: the argument check (fme_extern_host.h); *run: enqueue.
static int extern_enter(fme_ctx* c, int rq, int n, const char* name, bool* run) {
  *run = false;
  if (rq == FME_E_STATE) return fail(rq, "%s: NN input rows are bound (fme_set_nn_inputs): the inputs are the caller's", name);
  if (rq < 0) return fail(rq, "%s: bad argument (n = %d)", name, n);
  if (rq == 0) {
    HIP_TRY(hipSetDevice(c->device));
    *run = true;
  }
  return FME_OK;
}

// ---- candidate-set refinement (include/fme_among.h) -----------------------------------------------
// The among batch is at_batch with a list per job; the top-K batch is the inputs batch followed by
// the ranking and the among evaluation inside one scaffolded batch.  Their profiling events: [0] /
// [1] around k_front, [2] behind the EMI kernel, [3] the rows kernel, [4] the ranking, [5] the
// evaluation.
static int among_events(fme_ctx* c) {
  if (c->profiling)
    for (auto& e : c->ev_among)
      if (!e) HIP_TRY(hipEventCreate(&e.h));
  c->among_timed = false;   // until the call is enqueued in full
  return FME_OK;
}

static AmongArgs among_args(const fme_ctx* c, const Batch& b, const fme_nn_row* d_rows, const uint8_t* d_cand, int k,
                            fme_result* d_res, fme_mv_result* d_mv, uint32_t* d_cost, bool topk) {
  AmongArgs x{};
  x.d = direct_args(c, b);
  x.d.a.res = d_res;
  x.d.mv_out = d_mv;
  x.rows = d_rows;
  x.cand = d_cand;
  x.cand_cost = d_cost;
  x.refused = c->d_am_refused.p;
  x.k = k;
  x.status = FME_RES_NN_DIRECT | FME_RES_NN_AMONG | (topk ? 0u : FME_RES_NN_EXTERN);
  x.row_status = topk ? 1 : 0;
  x.n = b.a.n;
  x.bit_depth = c->cfg.bit_depth;
  return x;
}

// k_front -> EMI kernel unless the caller brought rows -> evaluation over the caller's lists.  d_res:
// the full records (with d_mv and no rows: context-internal ones the EMI kernel writes; with d_mv and
// rows: null).  The NN state is not touched.
static int among_batch(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cand, int k,
                       fme_result* d_res, fme_mv_result* d_mv, uint32_t* d_cost, int n, hipStream_t s) {
  HIP_TRY(c->d_am_refused.reserve(1));
  const bool prof = c->profiling;
  const Event* ev = c->ev_among;
  FME_TRY(among_events(c));
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, nullptr, nullptr, d_res, n, s, kOvForeign, 1, c->d_am_refused.p,
                      prof ? ev[0] : nullptr, prof ? ev[1] : nullptr, &b));
  if (!d_rows) {
    HIP_TRY(launch_direct_emi(direct_args(c, b), s));
    if (prof) HIP_TRY(hipEventRecord(ev[2], s));
  }
  HIP_TRY(hipEventRecord(b.search_end, s));
  HIP_TRY(launch_among_eval(among_args(c, b, d_rows, d_cand, k, d_res, d_mv, d_cost, false), s));
  if (prof) HIP_TRY(hipEventRecord(ev[5], s));
  c->among_phases = d_rows ? 8u : 9u;
  c->among_timed = prof;
  FME_TRY(batch_end(c, s, b, false));
  c->ev_among_done = b.done;
  return FME_OK;
}

// The context's rows and candidates of a top-K batch: sized for max_jobs on first use.
static int topk_buffers(fme_ctx* c, int n, int k, bool own_cand) {
  const size_t cap = std::max<size_t>((size_t)n, (size_t)std::max(c->cfg.max_jobs, 0));
  HIP_TRY(c->d_am_rows.reserve(cap));
  if (own_cand) HIP_TRY(c->d_am_cand.reserve(cap * FME_AMONG_MAX));
  (void)k;
  return FME_OK;
}

// k_front -> EMI kernel (on d_rec, context-internal records) -> rows kernel (the NN state handed on
// as by the inputs batch) -> ranking -> evaluation with the rows into d_res / d_mv.
static int topk_batch(fme_ctx* c, const fme_job* d_jobs, fme_result* d_rec, fme_result* d_res, fme_mv_result* d_mv,
                      int k, uint8_t* d_cand, uint32_t* d_cost, int n, hipStream_t s) {
  HIP_TRY(c->d_am_refused.reserve(1));
  FME_TRY(topk_buffers(c, n, k, !d_cand));
  if (!d_cand) d_cand = c->d_am_cand.p;
  fme_nn_row* const d_rows = c->d_am_rows.p;
  const bool prof = c->profiling;
  const Event* ev = c->ev_among;
  FME_TRY(among_events(c));
  Batch b;
  FME_TRY(batch_begin(c, d_jobs, nullptr, nullptr, d_rec, n, s, kOvForeign, 1, c->d_am_refused.p,
                      prof ? ev[0] : nullptr, prof ? ev[1] : nullptr, &b));
  HIP_TRY(launch_direct_emi(direct_args(c, b), s));
  if (prof) HIP_TRY(hipEventRecord(ev[2], s));
  HIP_TRY(hipEventRecord(b.search_end, s));
  FME_TRY(hand_state_on(c, s, b));
  HIP_TRY(launch_nn_rows(b.a, b.w, d_rows, c->state_cur, false, s));
  if (prof) HIP_TRY(hipEventRecord(ev[3], s));
  HIP_TRY(launch_nn_rank(d_rows, c->d_nn.p, d_cand, k, n, s));
  if (prof) HIP_TRY(hipEventRecord(ev[4], s));
  HIP_TRY(launch_among_eval(among_args(c, b, d_rows, d_cand, k, d_res, d_mv, d_cost, true), s));
  if (prof) HIP_TRY(hipEventRecord(ev[5], s));
  c->among_phases = 15u;
  c->among_timed = prof;
  FME_TRY(batch_end(c, s, b, true));
  c->ev_among_done = b.done;
  return FME_OK;
}

// The families' common start: the argument check (fme_among_host.h); *run: enqueue.
static int among_enter(fme_ctx* c, int rq, int k, int n, const char* name, bool* run) {
  *run = false;
  if (rq == FME_E_STATE && c->nn_in)
    return fail(rq, "%s: NN input rows are bound (fme_set_nn_inputs): the inputs are the caller's", name);
  if (rq == FME_E_STATE) return fail(rq, "%s: needs nn_mode 1 with weights loaded", name);
  if (rq == FME_E_UNSUPPORTED) return fail(rq, "%s: the two-layer net only (nn_mode 1), not nn_mode 2", name);
  if (rq < 0) return fail(rq, "%s: bad argument (k = %d, n = %d)", name, k, n);
  if (rq == 0) {
    HIP_TRY(hipSetDevice(c->device));
    *run = true;
  }
  return FME_OK;
}

extern "C" {

int fme_nn_inputs(fme_ctx* c, const fme_job* jobs, fme_nn_row* rows, int n, void* stream) {
  bool run;
  FME_TRY(extern_enter(c, extern_inputs_request(c, jobs, rows, n, c && c->nn_in), n, "fme_nn_inputs", &run));
  if (!run) return FME_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(c->d_res.reserve(n));
  HIP_TRY(c->d_ext_rows.reserve(n));
  return host_batch(c, jobs, n, s, "fme_nn_inputs", rows, c->d_ext_rows.p, (size_t)n * sizeof(fme_nn_row),
                    [&] { return inputs_batch(c, c->d_jobs.p, c->d_res.p, c->d_ext_rows.p, n, s); });
}

int fme_nn_inputs_device(fme_ctx* c, const fme_job* d_jobs, fme_nn_row* d_rows, int n, void* stream) {
  bool run;
  FME_TRY(extern_enter(c, extern_inputs_request(c, d_jobs, d_rows, n, c && c->nn_in), n, "fme_nn_inputs_device", &run));
  if (!run) return FME_OK;
  fme_result* d_rec = nullptr;
  FME_TRY(slot_records(c, n, &d_rec));
  return inputs_batch(c, d_jobs, d_rec, d_rows, n, static_cast<hipStream_t>(stream));
}

int fme_refine_at(fme_ctx* c, const fme_job* jobs, const fme_nn_row* rows, const uint8_t* cls, fme_result* res, int n,
                  void* stream) {
  bool run;
  FME_TRY(extern_enter(c, extern_at_request(c, jobs, cls, res, n, c && c->nn_in), n, "fme_refine_at", &run));
  if (!run) return FME_OK;
  const int bad = extern_first_refused(jobs, rows, cls, n);
  if (bad >= 0)
    return fail(FME_E_INVALID, "fme_refine_at: job %d has class %d%s", bad, (int)cls[bad],
                extern_class_ok(cls[bad]) ? " and a row that is not its own" : " (0..48)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(c->d_jobs.reserve(n));
  HIP_TRY(c->d_res.reserve(n));
  HIP_TRY(c->d_ext_cls.reserve(n));
  if (rows) HIP_TRY(c->d_ext_rows.reserve(n));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_ext_cls.p, cls, (size_t)n, hipMemcpyHostToDevice, s));
  if (rows) HIP_TRY(hipMemcpyAsync(c->d_ext_rows.p, rows, (size_t)n * sizeof(fme_nn_row), hipMemcpyHostToDevice, s));
  FME_TRY(at_batch(c, c->d_jobs.p, rows ? c->d_ext_rows.p : nullptr, c->d_ext_cls.p, c->d_res.p, nullptr, n, s));
  // the rejected-job count first: an invalid batch leaves the caller's array as it was
  FME_TRY(check_rejected(c, s, "fme_refine_at", "with an unsupported PU size or unset picture/lambda/key"));
  HIP_TRY(hipMemcpy(res, c->d_res.p, (size_t)n * sizeof(fme_result), hipMemcpyDeviceToHost));
  return FME_OK;
}

int fme_refine_at_device(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cls,
                         fme_result* d_res, int n, void* stream) {
  bool run;
  FME_TRY(extern_enter(c, extern_at_request(c, d_jobs, d_cls, d_res, n, c && c->nn_in), n, "fme_refine_at_device", &run));
  return run ? at_batch(c, d_jobs, d_rows, d_cls, d_res, nullptr, n, static_cast<hipStream_t>(stream)) : FME_OK;
}

int fme_refine_at_mv_device(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cls,
                            fme_mv_result* d_out, int n, void* stream) {
  bool run;
  FME_TRY(extern_enter(c, extern_at_request(c, d_jobs, d_cls, d_out, n, c && c->nn_in), n, "fme_refine_at_mv_device", &run));
  if (!run) return FME_OK;
  fme_result* d_rec = nullptr;   // the EMI kernel's records; with rows nothing reads or writes them
  if (!d_rows) FME_TRY(slot_records(c, n, &d_rec));
  return at_batch(c, d_jobs, d_rows, d_cls, d_rec, d_out, n, static_cast<hipStream_t>(stream));
}

int fme_refine_at_status(fme_ctx* c) {
  if (!c) return fail(FME_E_INVALID, "fme_refine_at_status: null ctx");
  if (!c->ev_at_done) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev_at_done));
  int32_t v = 0;
  HIP_TRY(hipMemcpy(&v, c->d_ext_refused.p, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

int fme_extern_last_ms(fme_ctx* c, float ms[4]) {
  if (!c || !ms) return fail(FME_E_INVALID, "fme_extern_last_ms: null argument");
  if (!c->extern_timed) return fail(FME_E_STATE, "fme_extern_last_ms: no profiled batch of fme_nn_inputs* / fme_refine_at*");
  HIP_TRY(hipSetDevice(c->device));
  const Event* e = c->ev_extern;
  const unsigned ph = c->extern_phases;
  const int last = (ph & 4u) ? 4 : 3;
  HIP_TRY(hipEventSynchronize(e[last]));
  ms[0] = ms[1] = ms[2] = 0.f;
  if (ph & 1u) HIP_TRY(hipEventElapsedTime(&ms[0], e[1], e[2]));
  if (ph & 2u) HIP_TRY(hipEventElapsedTime(&ms[1], e[2], e[3]));
  if (ph & 4u) HIP_TRY(hipEventElapsedTime(&ms[2], e[(ph & 1u) ? 2 : 1], e[4]));
  HIP_TRY(hipEventElapsedTime(&ms[3], e[0], e[last]));
  return FME_OK;
}

int fme_refine_among(fme_ctx* c, const fme_job* jobs, const fme_nn_row* rows, const uint8_t* cand, int k, fme_result* res,
                     uint32_t* cand_cost, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_request(c, jobs, cand, k, res, n, c && c->nn_in), k, n, "fme_refine_among", &run));
  if (!run) return FME_OK;
  const int bad = among_first_refused(jobs, rows, cand, k, n);
  if (bad >= 0)
    return fail(FME_E_INVALID, "fme_refine_among: job %d has %s", bad,
                among_list_ok(cand + (size_t)bad * k, k) ? "a row that is not its own"
                                                         : "a list with a slot in 49..254 or no class at all");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t nk = (size_t)n * k;
  HIP_TRY(c->d_jobs.reserve(n));
  HIP_TRY(c->d_res.reserve(n));
  HIP_TRY(c->d_am_cand.reserve(nk));
  if (rows) HIP_TRY(c->d_am_rows.reserve(n));
  if (cand_cost) HIP_TRY(c->d_am_cost.reserve(nk));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_am_cand.p, cand, nk, hipMemcpyHostToDevice, s));
  if (rows) HIP_TRY(hipMemcpyAsync(c->d_am_rows.p, rows, (size_t)n * sizeof(fme_nn_row), hipMemcpyHostToDevice, s));
  FME_TRY(among_batch(c, c->d_jobs.p, rows ? c->d_am_rows.p : nullptr, c->d_am_cand.p, k, c->d_res.p, nullptr,
                      cand_cost ? c->d_am_cost.p : nullptr, n, s));
  // the rejected-job count first: an invalid batch leaves the caller's arrays as they were
  FME_TRY(check_rejected(c, s, "fme_refine_among", "with an unsupported PU size or unset picture/lambda/key"));
  HIP_TRY(hipMemcpy(res, c->d_res.p, (size_t)n * sizeof(fme_result), hipMemcpyDeviceToHost));
  if (cand_cost) HIP_TRY(hipMemcpy(cand_cost, c->d_am_cost.p, nk * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FME_OK;
}

int fme_refine_among_device(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cand, int k,
                            fme_result* d_res, uint32_t* d_cand_cost, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_request(c, d_jobs, d_cand, k, d_res, n, c && c->nn_in), k, n, "fme_refine_among_device", &run));
  return run ? among_batch(c, d_jobs, d_rows, d_cand, k, d_res, nullptr, d_cand_cost, n, static_cast<hipStream_t>(stream))
             : FME_OK;
}

int fme_refine_among_mv_device(fme_ctx* c, const fme_job* d_jobs, const fme_nn_row* d_rows, const uint8_t* d_cand, int k,
                               fme_mv_result* d_out, uint32_t* d_cand_cost, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_request(c, d_jobs, d_cand, k, d_out, n, c && c->nn_in), k, n, "fme_refine_among_mv_device", &run));
  if (!run) return FME_OK;
  fme_result* d_rec = nullptr;   // the EMI kernel's records; with rows nothing reads or writes them
  if (!d_rows) FME_TRY(slot_records(c, n, &d_rec));
  return among_batch(c, d_jobs, d_rows, d_cand, k, d_rec, d_out, d_cand_cost, n, static_cast<hipStream_t>(stream));
}

int fme_refine_among_status(fme_ctx* c) {
  if (!c) return fail(FME_E_INVALID, "fme_refine_among_status: null ctx");
  if (!c->ev_among_done) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev_among_done));
  int32_t v = 0;
  HIP_TRY(hipMemcpy(&v, c->d_am_refused.p, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

int fme_nn_rank_device(fme_ctx* c, const fme_nn_row* d_rows, uint8_t* d_cand, int k, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_rank_request(c, d_rows, d_cand, k, n, c ? c->cfg.nn_mode : 1, c && c->nn_loaded), k, n,
                      "fme_nn_rank_device", &run));
  if (!run) return FME_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool prof = c->profiling;
  const Event* ev = c->ev_among;
  FME_TRY(among_events(c));
  if (prof) HIP_TRY(hipEventRecord(ev[0], s));
  HIP_TRY(launch_nn_rank(d_rows, c->d_nn.p, d_cand, k, n, s));
  if (prof) HIP_TRY(hipEventRecord(ev[4], s));
  c->among_phases = 4u;
  c->among_timed = prof;
  return FME_OK;
}

int fme_refine_topk(fme_ctx* c, const fme_job* jobs, fme_result* res, int k, uint8_t* cand, uint32_t* cand_cost, int n,
                    void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_topk_request(c, jobs, res, k, n, c && c->nn_in, c ? c->cfg.nn_mode : 1, c && c->nn_loaded), k,
                      n, "fme_refine_topk", &run));
  if (!run) return FME_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t nk = (size_t)n * k;
  HIP_TRY(c->d_jobs.reserve(n));
  HIP_TRY(c->d_res.reserve(n));
  if (cand_cost) HIP_TRY(c->d_am_cost.reserve(nk));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  // the EMI kernel's records and the batch's own share c->d_res: the evaluation writes whole records
  // behind the rows kernel, the one reader of the EMI kernel's
  FME_TRY(topk_batch(c, c->d_jobs.p, c->d_res.p, c->d_res.p, nullptr, k, nullptr, cand_cost ? c->d_am_cost.p : nullptr, n, s));
  FME_TRY(check_rejected(c, s, "fme_refine_topk", "with an unsupported PU size or unset picture/lambda/key"));
  HIP_TRY(hipMemcpy(res, c->d_res.p, (size_t)n * sizeof(fme_result), hipMemcpyDeviceToHost));
  if (cand) HIP_TRY(hipMemcpy(cand, c->d_am_cand.p, nk, hipMemcpyDeviceToHost));
  if (cand_cost) HIP_TRY(hipMemcpy(cand_cost, c->d_am_cost.p, nk * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FME_OK;
}

int fme_refine_topk_device(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, int k, uint8_t* d_cand,
                           uint32_t* d_cand_cost, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_topk_request(c, d_jobs, d_res, k, n, c && c->nn_in, c ? c->cfg.nn_mode : 1, c && c->nn_loaded),
                      k, n, "fme_refine_topk_device", &run));
  // (the EMI kernel writes the caller's records, the evaluation overwrites them whole)
  return run ? topk_batch(c, d_jobs, d_res, d_res, nullptr, k, d_cand, d_cand_cost, n, static_cast<hipStream_t>(stream))
             : FME_OK;
}

int fme_refine_topk_mv_device(fme_ctx* c, const fme_job* d_jobs, fme_mv_result* d_out, int k, uint8_t* d_cand,
                              uint32_t* d_cand_cost, int n, void* stream) {
  bool run;
  FME_TRY(among_enter(c, among_topk_request(c, d_jobs, d_out, k, n, c && c->nn_in, c ? c->cfg.nn_mode : 1, c && c->nn_loaded),
                      k, n, "fme_refine_topk_mv_device", &run));
  if (!run) return FME_OK;
  fme_result* d_rec = nullptr;
  FME_TRY(slot_records(c, n, &d_rec));
  return topk_batch(c, d_jobs, d_rec, nullptr, d_out, k, d_cand, d_cand_cost, n, static_cast<hipStream_t>(stream));
}

int fme_among_last_ms(fme_ctx* c, float ms[5]) {
  if (!c || !ms) return fail(FME_E_INVALID, "fme_among_last_ms: null argument");
  if (!c->among_timed) return fail(FME_E_STATE, "fme_among_last_ms: no profiled among / rank / top-K call");
  HIP_TRY(hipSetDevice(c->device));
  const Event* e = c->ev_among;
  const unsigned ph = c->among_phases;
  const int last = (ph & 8u) ? 5 : 4;
  HIP_TRY(hipEventSynchronize(e[last]));
  ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
  if (ph & 1u) HIP_TRY(hipEventElapsedTime(&ms[0], e[1], e[2]));
  if (ph & 2u) HIP_TRY(hipEventElapsedTime(&ms[1], e[2], e[3]));
  if (ph & 4u) HIP_TRY(hipEventElapsedTime(&ms[2], e[(ph & 2u) ? 3 : 0], e[4]));
  if (ph & 8u) HIP_TRY(hipEventElapsedTime(&ms[3], e[(ph & 4u) ? 4 : (ph & 1u) ? 2 : 1], e[5]));
  HIP_TRY(hipEventElapsedTime(&ms[4], e[0], e[last]));
  return FME_OK;
}

int fme_refine_direct(fme_ctx* c, const fme_job* jobs, fme_result* res, int n, void* stream) {
  bool run;
  FME_TRY(direct_enter(c, jobs, res, n, "fme_refine_direct", &run));
  if (!run) return FME_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(c->d_res.reserve(n));
  return host_batch(c, jobs, n, s, "fme_refine_direct", res, c->d_res.p, (size_t)n * sizeof(fme_result),
                    [&] { return direct_batch(c, c->d_jobs.p, c->d_res.p, nullptr, n, s); });
}

int fme_refine_direct_device(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, int n, void* stream) {
  bool run;
  FME_TRY(direct_enter(c, d_jobs, d_res, n, "fme_refine_direct_device", &run));
  return run ? direct_batch(c, d_jobs, d_res, nullptr, n, static_cast<hipStream_t>(stream)) : FME_OK;
}

int fme_refine_direct_mv_device(fme_ctx* c, const fme_job* d_jobs, fme_mv_result* d_out, int n, void* stream) {
  bool run;
  FME_TRY(direct_enter(c, d_jobs, d_out, n, "fme_refine_direct_mv_device", &run));
  if (!run) return FME_OK;
  fme_result* d_res = nullptr;
  FME_TRY(slot_records(c, n, &d_res));
  return direct_batch(c, d_jobs, d_res, d_out, n, static_cast<hipStream_t>(stream));
}

int fme_refine_direct_last_ms(fme_ctx* c, float ms[4]) {
  if (!c || !ms) return fail(FME_E_INVALID, "fme_refine_direct_last_ms: null argument");
  if (!c->direct_timed) return fail(FME_E_STATE, "fme_refine_direct_last_ms: no profiled direct batch");
  HIP_TRY(hipSetDevice(c->device));
  const Event* e = c->ev_direct;
  HIP_TRY(hipEventSynchronize(e[4]));
  for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&ms[k], e[1 + k], e[2 + k]));
  HIP_TRY(hipEventElapsedTime(&ms[3], e[0], e[4]));
  return FME_OK;
}

int fme_refine_device(fme_ctx* c, const fme_job* d_jobs, fme_result* d_res, int n, void* stream) {
  if (!c || (n > 0 && (!d_jobs || !d_res))) return fail(FME_E_INVALID, "fme_refine_device: null argument");
  if (n < 0) return fail(FME_E_INVALID, "fme_refine_device: n = %d", n);
  if (n == 0) return FME_OK;
  return refine_batch(c, d_jobs, d_res, nullptr, n, static_cast<hipStream_t>(stream));
}

int fme_refine_mv_device(fme_ctx* c, const fme_job* d_jobs, fme_mv_result* d_out, int n, void* stream) {
  if (!c || (n > 0 && (!d_jobs || !d_out))) return fail(FME_E_INVALID, "fme_refine_mv_device: null argument");
  if (n < 0) return fail(FME_E_INVALID, "fme_refine_mv_device: n = %d", n);
  if (n == 0) return FME_OK;
  HIP_TRY(hipSetDevice(c->device));
  fme_result* d_res = nullptr;
  FME_TRY(slot_records(c, n, &d_res));
  return refine_batch(c, d_jobs, d_res, d_out, n, static_cast<hipStream_t>(stream));
}

// ---- packed jobs (include/fme.h fme_job_packed) -----------------------------------------------
int fme_pack_jobs(const fme_job* jobs, int n, fme_job_packed* out, int32_t* key_base) {
  if (n < 0 || (n > 0 && (!jobs || !out || !key_base))) return fail(FME_E_INVALID, "fme_pack_jobs: bad argument");
  const int waves = (n + FME_PACK_WAVE - 1) / FME_PACK_WAVE;
  for (int wv = 0; wv < waves; wv++) {
    int64_t next = -1;   // where the wave's next keyed block must start (-1: no keyed job yet)
    key_base[wv] = -1;
    const int e = std::min(n, (wv + 1) * FME_PACK_WAVE);
    for (int i = wv * FME_PACK_WAVE; i < e; i++) {
      const fme_job& j = jobs[i];
      const char* why = nullptr;
      if ((j.x & 3) || (j.y & 3) || (j.w & 3) || (j.h & 3) || j.w < 4 || j.w > 64 || j.h < 4 || j.h > 64)
        why = "PU off the 4x4 grid or not 4..64";
      else if (j.x >= 8192 || j.y >= 8192) why = "x or y >= 8192";
      else if (j.org_id >= 64 || j.ref_id >= 64 || j.lambda_id >= 32) why = "slot id >= 64 or lambda_id >= 32";
      else if (j.flags & ~15u) why = "unknown flags";
      else if (j.bits_in >= 64) why = "bits_in >= 64";
      else if (j.mv_x <= -32767 || j.mv_x >= 32766 || j.mv_y <= -32767 || j.mv_y >= 32766) why = "int16-extreme mv";
      else if (j.key_offset >= 0) {
        if (next < 0) key_base[wv] = j.key_offset;
        else if ((int64_t)j.key_offset != next) why = "key block not dense in job order within its wave";
        next = (int64_t)j.key_offset + (int64_t)j.w * j.h;
      }
      if (why) return fail(FME_E_UNSUPPORTED, "fme_pack_jobs: job %d: %s (use fme_job)", i, why);
      uint32_t rg = 0;
      if (j.mv_y - 1 >= j.lt_y) rg |= FME_PK_RANGE_TOP;
      if (j.mv_y + 1 <= j.rb_y) rg |= FME_PK_RANGE_BOTTOM;
      if (j.mv_x - 1 >= j.lt_x) rg |= FME_PK_RANGE_LEFT;
      if (j.mv_x + 1 <= j.rb_x) rg |= FME_PK_RANGE_RIGHT;
      fme_job_packed p;
      p.pu = (uint32_t)(j.x >> 2) | ((uint32_t)(j.y >> 2) << 11) | ((uint32_t)((j.w >> 2) - 1) << 22) |
             ((uint32_t)((j.h >> 2) - 1) << 26);
      p.ctl = (uint32_t)j.org_id | ((uint32_t)j.ref_id << 6) | ((uint32_t)j.lambda_id << 12) |
              ((uint32_t)j.flags << 17) | ((uint32_t)(j.key_offset >= 0) << 21) | (rg << 22) |
              ((uint32_t)j.bits_in << 26);
      p.mv_x = j.mv_x;
      p.mv_y = j.mv_y;
      p.mvp_x = j.mvp_x;
      p.mvp_y = j.mvp_y;
      out[i] = p;
    }
  }
  return FME_OK;
}

int fme_unpack_jobs(const fme_job_packed* packed, const int32_t* key_base, int n, fme_job* out) {
  if (n < 0 || (n > 0 && (!packed || !key_base || !out))) return fail(FME_E_INVALID, "fme_unpack_jobs: bad argument");
  int64_t next = 0;
  for (int i = 0; i < n; i++) {
    const fme_job_packed& p = packed[i];
    if (i % FME_PACK_WAVE == 0) next = key_base[i / FME_PACK_WAVE];
    fme_job j;
    j.x = (uint16_t)((p.pu & 2047u) * 4u);
    j.y = (uint16_t)(((p.pu >> 11) & 2047u) * 4u);
    j.w = (uint8_t)((((p.pu >> 22) & 15u) + 1u) * 4u);
    j.h = (uint8_t)((((p.pu >> 26) & 15u) + 1u) * 4u);
    j.org_id = (uint8_t)(p.ctl & 63u);
    j.ref_id = (uint8_t)((p.ctl >> 6) & 63u);
    j.lambda_id = (uint8_t)((p.ctl >> 12) & 31u);
    j.flags = (uint8_t)((p.ctl >> 17) & 15u);
    const uint32_t rg = (p.ctl >> 22) & 15u;
    j.bits_in = (uint16_t)(p.ctl >> 26);
    j.mv_x = p.mv_x;
    j.mv_y = p.mv_y;
    j.mvp_x = p.mvp_x;
    j.mvp_y = p.mvp_y;
    j.lt_x = (int16_t)(p.mv_x - ((rg & FME_PK_RANGE_LEFT) ? 1 : 0));
    j.rb_x = (int16_t)(p.mv_x + ((rg & FME_PK_RANGE_RIGHT) ? 1 : 0));
    j.lt_y = (int16_t)(p.mv_y - ((rg & FME_PK_RANGE_TOP) ? 1 : 0));
    j.rb_y = (int16_t)(p.mv_y + ((rg & FME_PK_RANGE_BOTTOM) ? 1 : 0));
    if ((p.ctl >> 21) & 1u) {
      j.key_offset = (int32_t)next;
      next += (int64_t)j.w * j.h;
    } else {
      j.key_offset = -1;
    }
    out[i] = j;
  }
  return FME_OK;
}

static int refine_packed(fme_ctx* c, const fme_job_packed* d_jobs, const int32_t* d_key_base, fme_result* d_res,
                         fme_mv_result* d_mv, int n, void* stream, const char* fn) {
  if (!c || (n > 0 && (!d_jobs || !d_key_base || !(d_res || d_mv)))) return fail(FME_E_INVALID, "%s: null argument", fn);
  if (n < 0) return fail(FME_E_INVALID, "%s: n = %d", fn, n);
  if (n == 0) return FME_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (!d_res) FME_TRY(slot_records(c, n, &d_res));
  return refine_batch(c, nullptr, d_res, d_mv, n, static_cast<hipStream_t>(stream), d_jobs, d_key_base);
}

int fme_refine_packed_device(fme_ctx* c, const fme_job_packed* d_jobs, const int32_t* d_key_base, fme_result* d_res,
                             int n, void* stream) {
  if (c && n > 0 && !d_res) return fail(FME_E_INVALID, "fme_refine_packed_device: null argument");
  return refine_packed(c, d_jobs, d_key_base, d_res, nullptr, n, stream, "fme_refine_packed_device");
}

int fme_refine_mv_packed_device(fme_ctx* c, const fme_job_packed* d_jobs, const int32_t* d_key_base,
                                fme_mv_result* d_out, int n, void* stream) {
  if (c && n > 0 && !d_out) return fail(FME_E_INVALID, "fme_refine_mv_packed_device: null argument");
  return refine_packed(c, d_jobs, d_key_base, nullptr, d_out, n, stream, "fme_refine_mv_packed_device");
}

int fme_set_search_event(fme_ctx* c, void* event) {
  if (!c) return fail(FME_E_INVALID, "fme_set_search_event: null ctx");
  c->ev_search = static_cast<hipEvent_t>(event);
  return FME_OK;
}

int fme_set_search_reserve(fme_ctx* c, int workgroups) {
  if (!c || workgroups < 0 || workgroups > 4096) return fail(FME_E_INVALID, "fme_set_search_reserve: bad argument");
  c->search_reserve = workgroups;
  return FME_OK;
}

int fme_download_device(fme_ctx* c, const void* d_src, void* h_dst, size_t bytes, int workgroups, void* stream) {
  if (!c || (bytes && (!d_src || !h_dst))) return fail(FME_E_INVALID, "fme_download_device: null argument");
  if ((bytes & 15) || (reinterpret_cast<uintptr_t>(d_src) & 15) || (reinterpret_cast<uintptr_t>(h_dst) & 15))
    return fail(FME_E_INVALID, "fme_download_device: pointers and size must be 16-byte multiples");
  if (workgroups < 0 || workgroups > 1024) return fail(FME_E_INVALID, "fme_download_device: %d workgroups", workgroups);
  if (!bytes) return FME_OK;
  HIP_TRY(hipSetDevice(c->device));
  void* dst = nullptr;   // the device's address of the pinned host rows
  if (hipHostGetDevicePointer(&dst, h_dst, 0) != hipSuccess || !dst) {
    (void)hipGetLastError();
    return fail(FME_E_INVALID, "fme_download_device: h_dst is not pinned host memory");
  }
  HIP_TRY(launch_download(d_src, dst, bytes / 16, workgroups ? workgroups : 8, static_cast<hipStream_t>(stream)));
  return FME_OK;
}

// ---- copy-engine warm-up (fme_warm_copy_engines) ---------------------------------------------
// ROCclr submits each hipMemcpyAsync between host and device memory to one SDMA engine of the
// device; when a stream's previous engine is still busy it asks the HSA runtime for a free one
// (hsa_amd_memory_copy_engine_status), and the HSA runtime creates an engine's queue at its first
// use.  That creation blocked the submitting host thread for 5.6-7.5 ms each time a pipelined copy
// landed on an engine not used before (gpurun_out/r06a/env_logwait.log: "Query copy engine status
// ... free_engine_mask 0xfffe" -> copy_engine=0x2 -> a 6.7 ms host gap), and the device drained
// meanwhile.  Here every engine gets one small copy in each direction up front, through the HSA
// runtime HIP already initialised (its symbols resolved from the loaded library, no link
// dependency).
namespace {
struct HsaCopyApi {
  hsa_status_t (*iterate_agents)(hsa_status_t (*)(hsa_agent_t, void*), void*);
  hsa_status_t (*agent_get_info)(hsa_agent_t, hsa_agent_info_t, void*);
  hsa_status_t (*signal_create)(hsa_signal_value_t, uint32_t, const hsa_agent_t*, hsa_signal_t*);
  hsa_status_t (*signal_destroy)(hsa_signal_t);
  hsa_signal_value_t (*signal_wait)(hsa_signal_t, hsa_signal_condition_t, hsa_signal_value_t, uint64_t,
                                    hsa_wait_state_t);
  hsa_status_t (*copy_on_engine)(void*, hsa_agent_t, const void*, hsa_agent_t, size_t, uint32_t,
                                 const hsa_signal_t*, hsa_signal_t, hsa_amd_sdma_engine_id_t, bool);
};
bool hsa_copy_api(HsaCopyApi& a) {
  void* h = dlopen("libhsa-runtime64.so.1", RTLD_LAZY | RTLD_NOLOAD);
  if (!h) h = dlopen("libhsa-runtime64.so.1", RTLD_LAZY);
  if (!h) return false;
  a.iterate_agents = reinterpret_cast<decltype(a.iterate_agents)>(dlsym(h, "hsa_iterate_agents"));
  a.agent_get_info = reinterpret_cast<decltype(a.agent_get_info)>(dlsym(h, "hsa_agent_get_info"));
  a.signal_create = reinterpret_cast<decltype(a.signal_create)>(dlsym(h, "hsa_signal_create"));
  a.signal_destroy = reinterpret_cast<decltype(a.signal_destroy)>(dlsym(h, "hsa_signal_destroy"));
  a.signal_wait = reinterpret_cast<decltype(a.signal_wait)>(dlsym(h, "hsa_signal_wait_scacquire"));
  a.copy_on_engine = reinterpret_cast<decltype(a.copy_on_engine)>(dlsym(h, "hsa_amd_memory_async_copy_on_engine"));
  return a.iterate_agents && a.agent_get_info && a.signal_create && a.signal_destroy && a.signal_wait &&
         a.copy_on_engine;
}
struct AgentPick {
  const HsaCopyApi* api;
  uint32_t bdf, domain;
  bool have_gpu = false, have_cpu = false;
  hsa_agent_t gpu{}, cpu{};
};
hsa_status_t pick_agent(hsa_agent_t ag, void* data) {
  AgentPick* p = static_cast<AgentPick*>(data);
  hsa_device_type_t t;
  if (p->api->agent_get_info(ag, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
  if (t == HSA_DEVICE_TYPE_CPU && !p->have_cpu) {
    p->cpu = ag;
    p->have_cpu = true;
  } else if (t == HSA_DEVICE_TYPE_GPU && !p->have_gpu) {
    uint32_t bdf = 0, dom = 0;
    p->api->agent_get_info(ag, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf);
    p->api->agent_get_info(ag, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &dom);
    if (bdf == p->bdf && dom == p->domain) {
      p->gpu = ag;
      p->have_gpu = true;
    }
  }
  return HSA_STATUS_SUCCESS;
}
}  // namespace

int fme_warm_copy_engines(fme_ctx* c, int* engines) {
  if (!c) return fail(FME_E_INVALID, "fme_warm_copy_engines: null ctx");
  if (engines) *engines = 0;
  HIP_TRY(hipSetDevice(c->device));
  HsaCopyApi api{};
  if (!hsa_copy_api(api)) return fail(FME_E_DEVICE, "fme_warm_copy_engines: HSA runtime symbols not found");
  int bus = 0, dev = 0, dom = 0;
  HIP_TRY(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->device));
  HIP_TRY(hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, c->device));
  HIP_TRY(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, c->device));
  AgentPick pk{&api, (uint32_t)((bus << 8) | (dev << 3)), (uint32_t)dom};
  api.iterate_agents(pick_agent, &pk);
  if (!pk.have_gpu || !pk.have_cpu) return fail(FME_E_DEVICE, "fme_warm_copy_engines: HSA agents not found");
  uint32_t n_sdma = 0, n_xgmi = 0;
  api.agent_get_info(pk.gpu, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_NUM_SDMA_ENG), &n_sdma);
  api.agent_get_info(pk.gpu, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_NUM_SDMA_XGMI_ENG), &n_xgmi);
  const int n_eng = std::min(16, (int)(n_sdma + n_xgmi));
  constexpr size_t kBytes = 4096;
  void* d = nullptr;
  void* h = nullptr;
  HIP_TRY(hipMalloc(&d, kBytes));
  if (hipHostMalloc(&h, kBytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipFree(d);
    return fail(FME_E_NOMEM, "fme_warm_copy_engines: host buffer");
  }
  std::memset(h, 0, kBytes);
  int warmed = 0;
  for (int e = 0; e < n_eng; e++) {
    bool ok = true;
    for (int dir = 0; dir < 2 && ok; dir++) {   // host -> device, device -> host
      hsa_signal_t sig;
      if (api.signal_create(1, 0, nullptr, &sig) != HSA_STATUS_SUCCESS) {
        ok = false;
        break;
      }
      const auto eid = static_cast<hsa_amd_sdma_engine_id_t>(1u << e);
      const hsa_status_t st = dir == 0 ? api.copy_on_engine(d, pk.gpu, h, pk.cpu, kBytes, 0, nullptr, sig, eid, true)
                                       : api.copy_on_engine(h, pk.cpu, d, pk.gpu, kBytes, 0, nullptr, sig, eid, true);
      if (st == HSA_STATUS_SUCCESS)
        api.signal_wait(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
      else
        ok = false;
      api.signal_destroy(sig);
    }
    warmed += ok ? 1 : 0;
  }
  (void)hipHostFree(h);
  (void)hipFree(d);
  if (engines) *engines = warmed;
  return FME_OK;
}

int fme_refine_status(fme_ctx* c) {
  if (!c) return fail(FME_E_INVALID, "fme_refine_status: null ctx");
  if (!c->batch_issued) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev_done));
  int32_t v = 0;
  HIP_TRY(hipMemcpy(&v, &c->d_sched.p[c->last_ring].invalid, sizeof(v), hipMemcpyDeviceToHost));
  return v;
}

// Debugging aid for the tests of the front end (not declared in include/fme.h): what the last
// refinement batch's k_front left, read after waiting for the batch.  perm_out (may be null): the
// first perm_words words of perm; sched_out (may be null): the first sched_words int32 words of the
// Schedule (prefix[25], class_off[24], class_cnt[24], xq[8][25], invalid); *cap_out: the distance
// between two class regions of perm, in jobs.
int fme_debug_front(fme_ctx* c, int32_t* perm_out, long long perm_words, int32_t* sched_out, int sched_words,
                    int32_t* cap_out) {
  if (!c || !c->batch_issued) return fail(FME_E_STATE, "fme_debug_front: no batch issued");
  if (perm_words < 0 || (size_t)perm_words > c->perm[c->last_slot].cap || sched_words < 0 ||
      (size_t)sched_words * sizeof(int32_t) > sizeof(Schedule))
    return fail(FME_E_INVALID, "fme_debug_front: length");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev_done));
  if (perm_out && perm_words) HIP_TRY(hipMemcpy(perm_out, c->perm[c->last_slot].p, (size_t)perm_words * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (sched_out && sched_words) HIP_TRY(hipMemcpy(sched_out, c->d_sched.p + c->last_ring, (size_t)sched_words * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (cap_out) *cap_out = (int32_t)(c->perm[c->last_slot].cap / kNumClasses);
  return FME_OK;
}

// ---- integer motion estimation (xTZSearch / xPatternSearch) -----------------------------------
// classify (validation + class histogram, one host sync) -> scatter (jobs grouped by PU shape)
// -> one search launch per unit shape (fme_tz.hip) writing mv_x / mv_y (and ruiSAD) in place.
}  // extern "C"

// d_emi (may be null): also run the EMI square step of uni-pred EMI jobs and write the resulting
// integer MV there (the producer's m_integerMv2Nx2N), leaving jobs' mv_x / mv_y at the TZ best.
// d_nn_in (may be null): FME_TZ_RING jobs run the backups' square + ring and write their NN inputs.
int fme::tz_run(fme_ctx* c, fme_job* d_jobs, const fme_tz_ext* d_ext, uint32_t* d_sad, int n, void* stream,
                int16_t* d_emi, uint32_t* d_nn_in, int ext_stride) {
  if (!c || (n > 0 && (!d_jobs || !d_ext))) return fail(FME_E_INVALID, "fme_integer_search_device: null argument");
  if (n < 0) return fail(FME_E_INVALID, "fme_integer_search_device: n = %d", n);
  if (n == 0) return FME_OK;
  // The search groups its PUs by (unit-shape kernel, reference picture, CTU) on the device, each
  // group's search area read into LDS once (fme_tz.hip k_tz_staged): np groups per kernel, refused
  // here, before anything is planned or enqueued, when the bound pictures make too many.
  int cw = 0, ch = 0, npic = 0;   // CTU grid of the largest bound picture; reference ids < npic
  for (int i = 0; i < FME_MAX_PICTURES; i++)
    if (c->pics[i].luma) {
      cw = std::max(cw, (c->pics[i].width + 63) / 64);
      ch = std::max(ch, (c->pics[i].height + 63) / 64);
      npic = i + 1;
    }
  const long long np = (long long)npic * cw * ch;   // 0: no picture bound, every job fails k_classify
  if (np > kTzMaxPairs)
    return fail(FME_E_UNSUPPORTED, "fme_integer_search_device: %lld (picture slot, CTU) pairs (%d slots x %d x %d CTUs), the limit is %lld",
                np, npic, cw, ch, kTzMaxPairs);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FME_TRY(ensure_work(c, n));
  FME_TRY(sync_tables(c, s));
  // The integer search is planned like a refinement batch (kOvForeign): behind every batch in
  // flight, with a batch number of its own, so that its slot and counter block are nobody else's,
  // the block comes round zeroed again (its scatter zeroes the block of the batch after next, as
  // k_front does) and the batches after it wait for its events, both recorded at its end.  It
  // reads copy 0 of the tables.
  Batch bt;
  FME_TRY(batch_open(c, s, kOvForeign, &bt));
  BatchArgs& a = bt.a;
  a = batch_args(c, d_jobs, n);
  a.nn_in = c->nn_in;   // FME_JOB_NN_IN jobs (the B producer's bi rounds) pass k_classify with their rows
  a.nn_in_cap = c->nn_in_cap;
  const WorkBufs& w = bt.w;
  FME_TRY(c->tz_timer.ensure(c));   // (its events are made before the blocks are in doubt)
  // in doubt until everything is enqueued (an invalid job ends the call after the first pass)
  overlap_begin(c->ov);
  HIP_TRY(launch_classify(a, w, s));
  HIP_TRY(hipMemcpyAsync(c->h_counts, w.counts, kCountWords * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c->h_counts[kNumClasses] > 0)
    return fail(FME_E_INVALID, "fme_integer_search_device: %d job(s) with an unsupported PU size or unset picture/lambda/key",
                c->h_counts[kNumClasses]);
  const bool keyed = c->h_counts[kKeyedWord] > 0;
  HIP_TRY(launch_scatter(a, w, c->sched_p, s));   // with its own class offsets (the schedule goes unused)
  TzArgs ta{};
  ta.a = a;
  ta.perm = w.perm;
  ta.jobs_out = d_jobs;
  ta.ext = d_ext;
  ta.ext_stride = ext_stride;
  ta.sad = d_sad;
  ta.emi_mv = d_emi;
  ta.nn_in = d_nn_in;
  FME_TRY(c->tz_timer.begin(c, s));
  // the three unit-shape kernels are latency-bound and independent: 4x8 and 8x4 units on the two
  // auxiliary streams, 8x8 units on the caller's stream, joined before returning
  // the integer search's own auxiliary streams (the refinement batch uses none)
  if (!c->aux) HIP_TRY(hipStreamCreateWithFlags(&c->aux.h, hipStreamNonBlocking));
  if (!c->aux2) HIP_TRY(hipStreamCreateWithFlags(&c->aux2.h, hipStreamNonBlocking));
  if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming));
  if (!c->ev_join) HIP_TRY(hipEventCreateWithFlags(&c->ev_join.h, hipEventDisableTiming));
  if (!c->ev_join2) HIP_TRY(hipEventCreateWithFlags(&c->ev_join2.h, hipEventDisableTiming));
  // the groups (np > 0 here: a job that passed k_classify names a bound picture)
  const size_t words = 8 + 12 * (size_t)np;
  if (c->d_tzp.cap < words || c->d_tzp_perm.cap < (size_t)n) {
    FME_TRY(drain_ctx(c));   // no launch of an earlier call still reads the old buffers
    HIP_TRY(c->d_tzp.reserve(words));
    HIP_TRY(c->d_tzp_perm.reserve(n));
  }
  TzPairs tp{};
  int32_t* b = c->d_tzp.p;
  tp.nseg = b;
  tp.cnt = b + 8;
  tp.cursor = tp.cnt + 3 * np;
  tp.off = tp.cursor + 3 * np;
  tp.seg = tp.off + 3 * np;
  tp.perm = c->d_tzp_perm.p;
  tp.np = (int32_t)np;
  tp.cw = cw;
  tp.ch = ch;
  HIP_TRY(hipMemsetAsync(b, 0, (8 + 3 * (size_t)np) * sizeof(int32_t), s));
  HIP_TRY(launch_tz_pairs(ta, tp, w.cls, n, s));
  HIP_TRY(hipEventRecord(c->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
  HIP_TRY(hipStreamWaitEvent(c->aux2, c->ev_fork, 0));
  HIP_TRY(launch_tz_staged(ta, tp, 0, keyed, c->cfg.bit_depth, c->aux));
  HIP_TRY(launch_tz_staged(ta, tp, 1, keyed, c->cfg.bit_depth, c->aux2));
  HIP_TRY(launch_tz_staged(ta, tp, 2, keyed, c->cfg.bit_depth, s));
  HIP_TRY(hipEventRecord(c->ev_join, c->aux));
  HIP_TRY(hipEventRecord(c->ev_join2, c->aux2));
  HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
  HIP_TRY(hipStreamWaitEvent(s, c->ev_join2, 0));
  FME_TRY(c->tz_timer.end(c, s));
  HIP_TRY(hipEventRecord(bt.search_end, s));
  return batch_close(c, s, bt);
}

static int tz_run_host(fme_ctx* c, fme_job* jobs, const fme_tz_ext* ext, uint32_t* sad, int n, void* stream,
                       int16_t* emi, uint32_t* nn_in = nullptr, int ext_stride = (int)sizeof(fme_tz_ext)) {
  if (!c || (n > 0 && (!jobs || !ext))) return fail(FME_E_INVALID, "fme_integer_search: null argument");
  if (n <= 0) return n == 0 ? FME_OK : fail(FME_E_INVALID, "fme_integer_search: n = %d", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(c->d_jobs.reserve(n));
  HIP_TRY(c->d_tz_ext.reserve(((size_t)n * ext_stride + sizeof(fme_tz_ext) - 1) / sizeof(fme_tz_ext)));
  HIP_TRY(c->d_tz_sad.reserve(n));
  if (emi) HIP_TRY(c->d_tz_emi.reserve((size_t)2 * n));
  if (nn_in) HIP_TRY(c->d_tz_nn_in.reserve((size_t)9 * n));
  HIP_TRY(hipMemcpyAsync(c->d_jobs.p, jobs, (size_t)n * sizeof(fme_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_tz_ext.p, ext, (size_t)n * ext_stride, hipMemcpyHostToDevice, s));
  // rows of jobs without FME_TZ_RING are left untouched: start from the caller's values
  if (nn_in) HIP_TRY(hipMemcpyAsync(c->d_tz_nn_in.p, nn_in, (size_t)9 * n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  int rc = tz_run(c, c->d_jobs.p, c->d_tz_ext.p, c->d_tz_sad.p, n, stream, emi ? c->d_tz_emi.p : nullptr,
                  nn_in ? c->d_tz_nn_in.p : nullptr, ext_stride);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(jobs, c->d_jobs.p, (size_t)n * sizeof(fme_job), hipMemcpyDeviceToHost, s));
  if (sad) HIP_TRY(hipMemcpyAsync(sad, c->d_tz_sad.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (emi) HIP_TRY(hipMemcpyAsync(emi, c->d_tz_emi.p, (size_t)n * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  if (nn_in) HIP_TRY(hipMemcpyAsync(nn_in, c->d_tz_nn_in.p, (size_t)9 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

extern "C" {

int fme_integer_search_device(fme_ctx* c, fme_job* d_jobs, const fme_tz_ext* d_ext, uint32_t* d_sad, int n,
                              void* stream) {
  return tz_run(c, d_jobs, d_ext, d_sad, n, stream, nullptr);
}

int fme_integer_search(fme_ctx* c, fme_job* jobs, const fme_tz_ext* ext, uint32_t* sad, int n, void* stream) {
  return tz_run_host(c, jobs, ext, sad, n, stream, nullptr);
}

int fme_integer_search2_device(fme_ctx* c, fme_job* d_jobs, const fme_tz_ext2* d_ext, uint32_t* d_sad, int n,
                               void* stream) {
  return tz_run(c, d_jobs, reinterpret_cast<const fme_tz_ext*>(d_ext), d_sad, n, stream, nullptr, nullptr,
                (int)sizeof(fme_tz_ext2));
}

int fme_integer_search2(fme_ctx* c, fme_job* jobs, const fme_tz_ext2* ext, uint32_t* sad, int n, void* stream) {
  return tz_run_host(c, jobs, reinterpret_cast<const fme_tz_ext*>(ext), sad, n, stream, nullptr, nullptr,
                     (int)sizeof(fme_tz_ext2));
}

int fme_integer_search_ring_device(fme_ctx* c, fme_job* d_jobs, const fme_tz_ext* d_ext, uint32_t* d_sad,
                                   uint32_t* d_nn_in, int n, void* stream) {
  if (!d_nn_in && n > 0) return fail(FME_E_INVALID, "fme_integer_search_ring_device: null nn_in");
  return tz_run(c, d_jobs, d_ext, d_sad, n, stream, nullptr, d_nn_in);
}

int fme_integer_search_ring(fme_ctx* c, fme_job* jobs, const fme_tz_ext* ext, uint32_t* sad, uint32_t* nn_in,
                            int n, void* stream) {
  if (!nn_in && n > 0) return fail(FME_E_INVALID, "fme_integer_search_ring: null nn_in");
  return tz_run_host(c, jobs, ext, sad, n, stream, nullptr, nn_in);
}

int fme_integer_search_last_ms(fme_ctx* c, float* ms) {
  return timer_last_ms(c, &fme_ctx::tz_timer, "fme_integer_search_last_ms", "integer search", ms);
}

static int refine_host(fme_ctx* c, const fme_job* jobs, fme_result* res, fme_mv_result* mv, int n, void* stream,
                       const char* name) {
  if (!c || (n > 0 && (!jobs || (!res && !mv)))) return fail(FME_E_INVALID, "%s: null argument", name);
  if (n <= 0) return n == 0 ? FME_OK : fail(FME_E_INVALID, "%s: n = %d", name, n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(c->d_res.reserve(n));
  if (mv) HIP_TRY(c->d_mv.reserve(n));
  return host_batch(c, jobs, n, s, name, mv ? (void*)mv : (void*)res, mv ? (const void*)c->d_mv.p : (const void*)c->d_res.p,
                    (size_t)n * (mv ? sizeof(fme_mv_result) : sizeof(fme_result)),
                    [&] { return refine_batch(c, c->d_jobs.p, c->d_res.p, mv ? c->d_mv.p : nullptr, n, s); });
}

int fme_refine(fme_ctx* c, const fme_job* jobs, fme_result* res, int n, void* stream) {
  return refine_host(c, jobs, res, nullptr, n, stream, "fme_refine");
}

int fme_refine_mv(fme_ctx* c, const fme_job* jobs, fme_mv_result* out, int n, void* stream) {
  return refine_host(c, jobs, nullptr, out, n, stream, "fme_refine_mv");
}

// The deeper nets' single NN_pred call: its completion word in pinned, device-mapped host memory.
static int ensure_stage(fme_ctx* c) {
  if (c->stage) return FME_OK;
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, sizeof(SingleStage), hipHostMallocMapped));
  c->stage = static_cast<SingleStage*>(p);
  void* d = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&d, p, 0));
  c->stage_dev = static_cast<uint8_t*>(d);
  HIP_TRY(hipStreamCreateWithFlags(&c->single_stream.h, hipStreamNonBlocking));
  std::memset(c->stage, 0, sizeof(SingleStage));
  return FME_OK;
}

static int class_of(int w, int h) {
  for (int k = 0; k < kNumClasses; k++)
    if (kClassW[k] == w && kClassH[k] == h) return k;
  return -1;
}

// Wait for a single-PU kernel's completion word (written after its results, system-scope release)
// instead of synchronising the stream; the stream is queried now and then so a kernel that ended
// without writing it (a device error) is reported, not waited on forever.
static int single_wait(fme_ctx* c, uint32_t seq) {
  volatile uint32_t* f = &c->stage->flag;
  for (long it = 1; *f != seq; it++) {
    __builtin_ia32_pause();
    if ((it & 1023) == 0) {
      const hipError_t q = hipStreamQuery(c->single_stream);
      if (q != hipErrorNotReady && *f != seq) {
        if (q != hipSuccess) return fail(FME_E_DEVICE, "single-PU kernel: %s", hipGetErrorString(q));
        return fail(FME_E_DEVICE, "single-PU kernel ended without its completion word");
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return FME_OK;
}

// ---- the single-call server (fme_server.hip) ----------------------------------------------------
// One resident workgroup serves fme_frac_dif_single and the master net's fme_nn_pred_single: the
// host writes the request into the mailbox (pinned, device-mapped), releases req_seq and spins on
// the answer block res.  An instance exits after kSrvIdleUs without a call or kSrvLifeMs of life (or on `stop`)
// and writes its epoch to `stopped`; a call that finds its instance gone relaunches one, which
// serves the pending request.
constexpr uint64_t kSrvIdleUs = 2000;
constexpr uint64_t kSrvLifeMs = 100;

static int srv_open(fme_ctx* c) {
  if (c->box) return FME_OK;
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, sizeof(SrvBox), hipHostMallocMapped));
  std::memset(p, 0, sizeof(SrvBox));
  c->box = static_cast<SrvBox*>(p);
  void* d = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&d, p, 0));
  c->box_dev = static_cast<SrvBox*>(d);
  HIP_TRY(hipStreamCreateWithFlags(&c->srv_stream.h, hipStreamNonBlocking));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0)
    c->srv_khz = (uint64_t)khz;
  return FME_OK;
}

static int srv_launch(fme_ctx* c) {
  if (c->srv_orphan) {   // never two instances on one mailbox: relaunch only once the old one has left
    const hipError_t q = hipStreamQuery(c->srv_stream);
    if (q == hipErrorNotReady)
      return fail(FME_E_DEVICE, "single-call server: the instance that timed out is still running");
    (void)hipGetLastError();
    c->srv_orphan = false;
  }
  __atomic_store_n(&c->box->req[0][3], 0u, __ATOMIC_RELEASE);
  const uint32_t epoch = ++c->srv_epoch;
  c->srv_nn_gen = c->nn_gen;
  HIP_TRY(launch_server(c->box_dev, c->nn_loaded ? c->d_nn.p : nullptr, c->srv_done, epoch,
                        kSrvIdleUs * c->srv_khz / 1000, kSrvLifeMs * c->srv_khz, c->cfg.bit_depth, c->srv_stream));
  c->srv_running = true;
  return FME_OK;
}

// The running instance's end: its `stopped` word (or a device error on its stream).
// Host-side bound of a wait on the server (a call, or its stop): far above any call's work (a 64x64
// FracDIF takes ~0.1 ms, an instance lives 100 ms), so only a server that never answers reaches it.
constexpr double kSrvWaitLimitS = 2.0;
static bool srv_waited_too_long(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kSrvWaitLimitS;
}

static int srv_join(fme_ctx* c) {
  volatile uint32_t* st = &c->box->stopped;
  const auto t0 = std::chrono::steady_clock::now();
  for (long it = 1; *st != c->srv_epoch; it++) {
    __builtin_ia32_pause();
    if ((it & 1023) == 0) {
      const hipError_t q = hipStreamQuery(c->srv_stream);
      if (q != hipErrorNotReady && *st != c->srv_epoch) {
        c->srv_running = false;
        if (q != hipSuccess) return fail(FME_E_DEVICE, "single-call server: %s", hipGetErrorString(q));
        return fail(FME_E_DEVICE, "single-call server ended without its stop word");
      }
      if (srv_waited_too_long(t0)) {
        c->srv_running = false;
        c->srv_orphan = true;   // srv_launch waits for it to leave srv_stream before a relaunch
        return fail(FME_E_DEVICE, "single-call server: no stop word after %.1f s", kSrvWaitLimitS);
      }
    }
  }
  c->srv_running = false;
  HIP_TRY(hipStreamSynchronize(c->srv_stream));
  return FME_OK;
}

static int srv_stop(fme_ctx* c) {
  if (!c->srv_running) return FME_OK;
  __atomic_store_n(&c->box->req[0][3], 1u, __ATOMIC_RELEASE);
  return srv_join(c);
}

// One call: the request fields and payload are in c->box already.
static int srv_call(fme_ctx* c, bool uses_nn) {
  int rc = FME_OK;
  if (c->srv_running && uses_nn && c->srv_nn_gen != c->nn_gen) rc = srv_stop(c);
  if (!rc && !c->srv_running) rc = srv_launch(c);
  if (rc) return rc;
  const uint32_t seq = c->srv_done + 1;
  __atomic_store_n(&c->box->req[0][0], seq, __ATOMIC_RELEASE);
  volatile uint32_t* done = &c->box->res[0];
  volatile uint32_t* st = &c->box->stopped;
  const auto t0 = std::chrono::steady_clock::now();
  for (long it = 1; *done != seq; it++) {
    __builtin_ia32_pause();
    if (*st == c->srv_epoch && *done != seq) {   // the instance left before it saw the call
      c->srv_running = false;
      HIP_TRY(hipStreamSynchronize(c->srv_stream));
      if (srv_waited_too_long(t0))
        return fail(FME_E_DEVICE, "single-call server: call %u unanswered after %.1f s", seq, kSrvWaitLimitS);
      FME_TRY(srv_launch(c));
    } else if ((it & 4095) == 0) {
      const hipError_t q = hipStreamQuery(c->srv_stream);
      if (q != hipErrorNotReady && q != hipSuccess) {
        c->srv_running = false;
        return fail(FME_E_DEVICE, "single-call server: %s", hipGetErrorString(q));
      }
      if (srv_waited_too_long(t0)) {   // stop the instance (it exits within its lifetime) and give up
        __atomic_store_n(&c->box->req[0][3], 1u, __ATOMIC_RELEASE);
        if (srv_join(c) != FME_OK) c->srv_orphan = true;
        c->srv_running = false;
        return fail(FME_E_DEVICE, "single-call server: call %u unanswered after %.1f s", seq, kSrvWaitLimitS);
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  c->srv_done = seq;
  return FME_OK;
}

// xPatternSearchFracDIF for one PU, as TEncSearch calls it: the key block (pcPatternKey, HM Pel)
// and the reference window around the integer MV (rows -4..h+3, columns -4..w+3 of the padded
// picture) go into the server's mailbox; the MV predictor is shifted by 4*mv_int so that every
// MV-cost argument (xPatternRefinement's (cMvTest << scale) - pred) is unchanged.
// Both bit depths go through the same mailbox: the context's depth picks the server instance
// (k_server<8> / k_server<10>) and the window's sample size (srv_pack_frac, fme_srv_pack.h), so
// the caller's pictures, lambdas, keys and NN state are untouched at either depth.
int fme_frac_dif_single(fme_ctx* c, int lossless, const int16_t* key, int key_stride, int w, int h,
                        const int16_t* ref, int ref_stride, int mv_int_x, int mv_int_y, int mvp_x,
                        int mvp_y, double motion_lambda, int16_t* half_xy, int16_t* qtr_xy,
                        uint32_t* cost) {
  if (!c || !key || !ref || !half_xy || !qtr_xy || !cost) return fail(FME_E_INVALID, "fme_frac_dif_single: null argument");
  const int cls = class_of(w, h);
  if (cls < 0) return fail(FME_E_UNSUPPORTED, "fme_frac_dif_single: %dx%d", w, h);
  const int px = mvp_x - 4 * mv_int_x, py = mvp_y - 4 * mv_int_y;
  if (px < -32768 || px > 32767 || py < -32768 || py > 32767) return fail(FME_E_INVALID, "fme_frac_dif_single: predictor out of range");
  HIP_TRY(hipSetDevice(c->device));
  FME_TRY(srv_open(c));
  SrvBox* b = c->box;
  // request blocks, payload, shape and predictor; srv_call publishes the sequence word
  srv_pack_frac(b, c->srv_done + 1, c->cfg.bit_depth, lossless || !c->cfg.use_hadamard, c->srv_marks, key, key_stride, w,
                h, ref, ref_stride, mv_int_x, mv_int_y, px, py, motion_lambda);
  FME_TRY(srv_call(c, false));
  const uint32_t hq = b->res[2];
  half_xy[0] = (int16_t)(int8_t)(hq & 0xFF);
  half_xy[1] = (int16_t)(int8_t)((hq >> 8) & 0xFF);
  qtr_xy[0] = (int16_t)(int8_t)((hq >> 16) & 0xFF);
  qtr_xy[1] = (int16_t)(int8_t)(hq >> 24);
  *cost = b->res[1];
  return FME_OK;
}

int fme_nn_pred_single(fme_ctx* c, const uint32_t* e, uint32_t cc, int pu_h, int pu_w, int* nn_class, int16_t* out4) {
  if (!c || !e || !nn_class) return fail(FME_E_INVALID, "fme_nn_pred_single: null argument");
  const bool deep = c->cfg.nn_mode == 2;
  if (deep ? !c->net_loaded : !c->nn_loaded) return fail(FME_E_STATE, "fme_nn_pred_single: no weights loaded");
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (!deep) {   // the master net: the server, weights in its LDS
    FME_TRY(srv_open(c));
    const uint32_t in[12] = {e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], cc, (uint32_t)pu_h, (uint32_t)pu_w, 0u};
    const uint32_t seq = c->srv_done + 1;   // the call's sequence number (srv_call)
    for (int b = 1; b < 5; b++) {   // each block's inputs, then its sequence word
      for (int k = 0; k < 3; k++) c->box->req[b][1 + k] = in[3 * (b - 1) + k];
      __atomic_store_n(&c->box->req[b][0], seq, __ATOMIC_RELEASE);
    }
    c->box->req[0][1] = kSrvNn | (c->srv_marks ? (uint32_t)kSrvMarks : 0u);
    FME_TRY(srv_call(c, true));
    *nn_class = (int)c->box->res[1];
  } else {
  // a resident server (a FracDIF call just before) would hold this launch up on a hardware queue
  // its stream shares until its idle exit: stop it first, as the batch entry points do
  rc = srv_stop(c);
  if (!rc) rc = ensure_stage(c);
  if (rc) return rc;
  // inputs in the kernel argument, the class and the completion word through mapped host memory:
  // one launch, a spin on the completion word
  NnIn11 in{};
  for (int s = 0; s < 8; s++) in.v[s] = e[s];
  in.v[8] = cc;
  in.v[9] = (uint32_t)pu_h;
  in.v[10] = (uint32_t)pu_w;
  int32_t* d_out = reinterpret_cast<int32_t*>(c->stage_dev + offsetof(SingleStage, nn_out));
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(c->stage_dev + offsetof(SingleStage, flag));
  const uint32_t seq = ++c->single_seq;
  HIP_TRY(launch_nn_deep_single(c->net, c->d_net.p, in, d_out, d_flag, seq, c->single_stream));
  FME_TRY(single_wait(c, seq));
  *nn_class = c->stage->nn_out[0];
  }
  const int cls = *nn_class;
  if (out4) {
    // MVX_HALF, MVX_QRTER, MVY_HALF, MVY_QRTER of the switch at TEncSearch.cpp:136-193:
    // the half/quarter split of the offset (cls % 7 - 3, cls / 7 - 3) with the quarter part
    // in {-1, 0, 1} and x = 2 * half + quarter.
    const int ox = cls % 7 - 3, oy = cls / 7 - 3;
    auto split = [](int o, int16_t& hf, int16_t& qt) {
      static const int8_t H[7] = {-1, -1, 0, 0, 0, 1, 1}, Q[7] = {-1, 0, -1, 0, 1, 0, 1};
      hf = H[o + 3];
      qt = Q[o + 3];
    };
    split(ox, out4[0], out4[1]);
    split(oy, out4[2], out4[3]);
  }
  return FME_OK;
}

int fme_single_last_device_us(fme_ctx* c, float* us, int count) {
  if (!c || (count > 0 && !us)) return fail(FME_E_INVALID, "fme_single_last_device_us: null argument");
  const double k = 1000.0 / (double)c->srv_khz;
  if (count > 1) c->srv_marks = true;   // checkpoints cost wall-clock reads: recorded once asked for
  for (int i = 0; i < count && i < 5; i++)
    us[i] = !c->box ? 0.0f : (float)((double)(i == 0 ? c->box->res[3] : c->box->marks[i - 1]) * k);
  return FME_OK;
}

int fme_search_kernel_of_shape(int width, int height) {
  for (int k = 0; k < kNumClasses; k++)
    if (kClassW[k] == width && kClassH[k] == height) {
      return 0;   // every shape runs in the lane kernel
    }
  return -1;
}

// ---- motion compensation ---------------------------------------------------------------------
static const char* mc_job_problem(const fme_ctx* c, const fme_mc_job& j, int width, int height) {
  return pred_task_problem(c, kPredMc, j.x, j.y, j.w, j.h, j.flags, j.ref_id, 0, width, height);
}

static int mc_launch(fme_ctx* c, const fme_mc_job* d_jobs, int n, uint8_t* y, int ys, uint8_t* cb, uint8_t* cr,
                     int cs, int width, int height, hipStream_t s) {
  FME_TRY(c->mc_invalid.zero(s));
  FME_TRY(sync_tables(c, s));
  if (!c->wp_init) {   // the default weights: 1 << 0, offset 0
    for (auto& l : c->h_wp)
      for (auto& p : l)
        for (auto& q : p) q = fme_wp_param{1, 0, 0, {0, 0, 0}};
    c->wp_init = true;
  }
  if (c->wp_dirty) {   // (pageable source: the runtime stages it before returning)
    HIP_TRY(c->d_mc_wp.reserve(sizeof(c->h_wp) / sizeof(fme_wp_param)));
    HIP_TRY(hipMemcpyAsync(c->d_mc_wp.p, c->h_wp, sizeof(c->h_wp), hipMemcpyHostToDevice, s));
    c->wp_dirty = false;
  }
  McArgs a{};
  a.wp = c->d_mc_wp.p;
  a.jobs = d_jobs;
  a.pics = c->d_pics.p;
  a.y = y;
  a.cb = cb;
  a.cr = cr;
  a.invalid = c->mc_invalid.d.p;
  a.n = n;
  a.y_stride = ys;
  a.c_stride = cs;
  a.width = width;
  a.height = height;
  a.bit_depth = c->cfg.bit_depth;   // 10: uint16 planes, strides in samples (k_mc<true>)
  FME_TRY(c->mc_timer.begin(c, s));
  HIP_TRY(launch_mc(a, s));
  return c->mc_timer.end(c, s);
}

static int mc_check_planes(const void* y, int ys, const void* cb, const void* cr, int cs, int width, int height) {
  if (!y || !cb || !cr) return fail(FME_E_INVALID, "motion compensation: null plane");
  if (width <= 0 || height <= 0 || (width & 1) || (height & 1) || ys < width || cs < width / 2)
    return fail(FME_E_INVALID, "motion compensation: geometry %dx%d strides %d/%d", width, height, ys, cs);
  return FME_OK;
}

int fme_motion_compensate(fme_ctx* c, const fme_mc_job* jobs, int n, uint8_t* y, int ys, uint8_t* cb, uint8_t* cr,
                          int cs, int width, int height, void* stream) {
  if (!c || (n > 0 && !jobs) || n < 0) return fail(FME_E_INVALID, "fme_motion_compensate: bad argument");
  if (int e = mc_check_planes(y, ys, cb, cr, cs, width, height)) return e;
  for (int i = 0; i < n; i++)
    if (const char* why = mc_job_problem(c, jobs[i], width, height))
      return fail(FME_E_INVALID, "fme_motion_compensate: job %d: %s", i, why);
  if (n == 0) return FME_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t bps = c->cfg.bit_depth > 8 ? 2 : 1;   // bytes per sample (10-bit: uint16 planes)
  const size_t ly = (size_t)width * height * bps, lc = ly / 4;
  HIP_TRY(c->d_mc_jobs.reserve(n));
  HIP_TRY(c->d_mc_planes.reserve(ly + 2 * lc));
  uint8_t* dy = c->d_mc_planes.p;
  uint8_t* dcb = dy + ly;
  uint8_t* dcr = dcb + lc;
  const int cw = width / 2, ch = height / 2;
  HIP_TRY(hipMemcpyAsync(c->d_mc_jobs.p, jobs, n * sizeof(fme_mc_job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpy2DAsync(dy, width * bps, y, ys * bps, width * bps, height, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpy2DAsync(dcb, cw * bps, cb, cs * bps, cw * bps, ch, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpy2DAsync(dcr, cw * bps, cr, cs * bps, cw * bps, ch, hipMemcpyHostToDevice, s));
  if (int e = mc_launch(c, c->d_mc_jobs.p, n, dy, width, dcb, dcr, cw, width, height, s)) return e;
  HIP_TRY(hipMemcpy2DAsync(y, ys * bps, dy, width * bps, width * bps, height, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpy2DAsync(cb, cs * bps, dcb, cw * bps, cw * bps, ch, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpy2DAsync(cr, cs * bps, dcr, cw * bps, cw * bps, ch, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FME_OK;
}

int fme_motion_compensate_device(fme_ctx* c, const fme_mc_job* d_jobs, int n, uint8_t* d_y, int ys, uint8_t* d_cb,
                                 uint8_t* d_cr, int cs, int width, int height, void* stream) {
  if (!c || (n > 0 && !d_jobs) || n < 0) return fail(FME_E_INVALID, "fme_motion_compensate_device: bad argument");
  if (int e = mc_check_planes(d_y, ys, d_cb, d_cr, cs, width, height)) return e;
  HIP_TRY(hipSetDevice(c->device));
  return mc_launch(c, d_jobs, n, d_y, ys, d_cb, d_cr, cs, width, height, static_cast<hipStream_t>(stream));
}

int fme_mc_invalid_count(fme_ctx* c) {
  // drains every stream the context used, where the other three wait for the last launch's: callers
  // have had that wider barrier since this replaced a device synchronisation, so it stays
  return invalid_count(c, &fme_ctx::mc_invalid, "fme_mc_invalid_count", true);
}

int fme_set_wp(fme_ctx* c, int list, int ref_id, const fme_wp_param* p) {
  if (!c || !p) return fail(FME_E_INVALID, "fme_set_wp: null argument");
  if (list < 0 || list > 1 || ref_id < 0 || ref_id >= FME_MAX_PICTURES)
    return fail(FME_E_INVALID, "fme_set_wp: list %d reference %d", list, ref_id);
  for (int k = 0; k < 3; k++)
    if (p[k].log2_denom > 7) return fail(FME_E_INVALID, "fme_set_wp: log2 denominator %d", (int)p[k].log2_denom);
  if (!c->wp_init) {
    for (auto& l : c->h_wp)
      for (auto& q : l)
        for (auto& r : q) r = fme_wp_param{1, 0, 0, {0, 0, 0}};
    c->wp_init = true;
  }
  for (int k = 0; k < 3; k++) c->h_wp[list][ref_id][k] = p[k];
  c->wp_dirty = true;
  return FME_OK;
}

int fme_mc_last_ms(fme_ctx* c, float* ms) {
  return timer_last_ms(c, &fme_ctx::mc_timer, "fme_mc_last_ms", "motion compensation", ms);
}

int fme_set_profiling(fme_ctx* c, int enable) {
  if (!c) return fail(FME_E_INVALID, "fme_set_profiling: null ctx");
  HIP_TRY(hipSetDevice(c->device));
  if (enable && !c->events_made) {
    for (auto& set : c->ev)
      for (auto& e : set) HIP_TRY(hipEventCreate(&e.h));
    c->events_made = true;
  }
  if (!enable) FME_TRY(harvest_events(c, true));
  c->profiling = enable != 0;
  return FME_OK;
}

int fme_last_timings(fme_ctx* c, float* ms, int count) {
  if (!c || !ms || count < 0) return fail(FME_E_INVALID, "fme_last_timings: null argument");
  HIP_TRY(hipSetDevice(c->device));
  FME_TRY(harvest_events(c, true));
  if (!c->timed) return fail(FME_E_STATE, "fme_last_timings: no profiled batch");
  for (int i = 0; i < count && i < FME_NUM_TIMINGS; i++) ms[i] = c->last_ms[i];
  return FME_OK;
}

int fme_accumulated_timings(fme_ctx* c, double* ms, int count, int reset) {
  if (!c || (count > 0 && !ms) || count < 0) return fail(FME_E_INVALID, "fme_accumulated_timings: null argument");
  HIP_TRY(hipSetDevice(c->device));
  FME_TRY(harvest_events(c, true));
  const int n = c->acc_batches;
  for (int i = 0; i < count && i < FME_NUM_TIMINGS; i++) ms[i] = c->acc_ms[i];
  if (reset) {
    for (double& v : c->acc_ms) v = 0.0;
    c->acc_batches = 0;
  }
  return n;
}

}  // extern "C"
