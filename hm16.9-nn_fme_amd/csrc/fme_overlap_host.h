// fme_overlap_host.h — the host's plan for a refinement batch that may overlap the batch before it
// (refine_batch, fme_api.cpp): which of the two work-buffer slots and which counter block the batch
// uses, and which earlier batches its stream has to wait for.  Plain C++: no HIP, so a CPU test
// can include it alone (tests/cpp/test_overlap_host.cpp).
//
// Batch k (counted over the batches a context has enqueued in full) uses slot k % 2 and counts in
// counter block k % kOvBlocks; k_front's last workgroup zeroes block (k + 2) % kOvBlocks.  With
// four blocks that block was last used by batch k - 2, which is over before batch k's k_front
// starts (the slot wait), and is next used by batch k + 2, whose k_front starts after batch k is
// over (its slot wait).  Three blocks would do for the zeroing alone (zero block k + 1), but then
// batch k + 1's k_front would have to be ordered after batch k's k_front by an event of its own;
// the fourth block costs 384 bytes.
//
// The only dependency between consecutive batches is the NN state that the tails hand on: the
// tail of batch k waits for the end of batch k - 1.  A batch with a feature that uses
// single-buffered context state (kOv* below) waits for every batch in flight before anything of
// it is enqueued, and so does the batch after it.  All waits are stream waits on the earlier
// batches' end events.  The integer search is planned like a batch with the feature kOvForeign: it
// takes a batch number, so its counter block comes round zeroed like any other and the batches
// after it wait for its end event.  A batch that the device rejects (an invalid job) is committed
// like any other: its kernels run and skip their work, and its k_front still zeroes its block.
// Only a batch abandoned on the host after its first launch (a failed launch) leaves the blocks
// in doubt; the next batch then fills them all behind a host-side drain of the context.
#pragma once

#include <cstdint>

namespace fme {

constexpr int kOvSlots = 2;
constexpr int kOvBlocks = 4;

// Features of a batch that serialise it behind every batch in flight.
enum : uint32_t {
  kOvKeys = 1u << 0,      // the key buffer was written since the last batch (one key buffer)
  kOvDeepNn = 1u << 1,    // nn_mode 2: its margin / logit / nn_in bindings are the caller's, one set
  kOvPx = 1u << 2,        // FME_MAIN10_SEARCH=px: the pixel kernels
  kOvStaged = 1u << 3,    // the context's own staging buffers (host entry points, the producers)
  kOvGrow = 1u << 4,      // a work buffer grows (freeing the old one waits for the device already;
                          // the bit keeps the rule in the plan, where the test can see it)
  kOvForeign = 1u << 5,   // not a refinement batch: the integer search, which takes a batch number,
                          // a slot and a counter block like one and ends with an end event like one
  kOvFill = 1u << 6,      // set by overlap_commit, not by callers: the batch began with a fill of all
                          // counter blocks on its stream, which the next batch must not overtake
};

struct OverlapPlan {
  int slot = 0;             // work-buffer slot
  int block = 0;            // counter block the batch counts in
  int block_zeroed = 0;     // counter block its k_front zeroes
  bool serial = false;      // wait for the end of batches k - 1 and k - 2 before anything is enqueued
  bool fill_blocks = false; // the counter blocks are not known to be zero: fill all of them first (serial)
  bool wait_slot = false;   // before k_front: the end of batch k - 2 (it ran on another stream)
  bool wait_prev_front = false;  // serial only: before anything, the end of batch k - 1 (another stream)
  bool wait_prev_tail = false;   // before the tail: the end of batch k - 1 (it ran on another stream)
};

struct OverlapState {
  long long seq = 0;                  // batches enqueued in full
  bool dirty = false;                 // a batch (or integer search) was abandoned half-way
  const void* stream[2] = {nullptr, nullptr};   // of batch seq - 1, seq - 2
  bool live[2] = {false, false};      // there is such a batch (and its end event)
  uint32_t prev_features = 0;         // of batch seq - 1
};

inline OverlapPlan overlap_plan(const OverlapState& st, const void* stream, uint32_t features) {
  OverlapPlan p;
  p.slot = (int)(st.seq % kOvSlots);
  p.block = (int)(st.seq % kOvBlocks);
  p.block_zeroed = (int)((st.seq + 2) % kOvBlocks);
  p.fill_blocks = st.dirty;
  // the batch after a serialised one waits as well: that one may use single-buffered state (the
  // context's staging buffers, the caller's NN bindings) until it ends
  p.serial = features != 0 || st.dirty || st.prev_features != 0;
  const bool other1 = st.live[0] && st.stream[0] != stream;
  const bool other2 = st.live[1] && st.stream[1] != stream;
  // batch k - 2 on this stream is over in stream order; on another stream its end event says when
  // (also where batch k - 1, on this stream, has already waited for it: a wait on an event that
  // has fired costs nothing on the device)
  p.wait_slot = other2;
  p.wait_prev_front = p.serial && other1;
  p.wait_prev_tail = other1 && !p.wait_prev_front;
  return p;
}

// Before the batch's first launch: whatever happens next, the blocks are in doubt until commit.
inline void overlap_begin(OverlapState& st) { st.dirty = true; }

// Every launch of the batch is enqueued and its end event recorded.  A batch that filled the
// counter blocks serialises the next one like a feature: the fill sits on this batch's stream, and
// a batch on another stream that started before it ran would have its block zeroed under it.
inline void overlap_commit(OverlapState& st, const void* stream, uint32_t features, const OverlapPlan& plan) {
  st.seq++;
  st.prev_features = features | (plan.fill_blocks ? (uint32_t)kOvFill : 0u);
  st.dirty = false;
  st.stream[1] = st.stream[0];
  st.live[1] = st.live[0];
  st.stream[0] = stream;
  st.live[0] = true;
}

}  // namespace fme
