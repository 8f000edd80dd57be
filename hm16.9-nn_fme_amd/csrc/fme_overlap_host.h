// fme_overlap_host.h — the host's plan for a refinement batch that may overlap the batches before
// it (refine_batch, fme_api.cpp): which work-buffer slot, which ring entry and which counter block
// the batch uses, and which earlier batches its stream has to wait for, and where.  Plain C++: no
// HIP, so a CPU test can include it alone (tests/cpp/test_overlap_host.cpp,
// tests/cpp/test_handover_host.cpp).
//
// A batch is three stages in stream order: the front end (k_front), the search, the tail.  Batch k
// (counted over the batches a context has enqueued in full) records two events: its search-end
// event behind the search launch, its end event behind the tail.  It uses
//   slot  k % kOvSlots   perm and cls (the front end writes them, the search reads them) and the
//                        internal record buffer of the *_mv_* entry points (search to tail);
//   ring  k % kOvRing    what the front end writes and the tail still reads: blk_agg / blk_prefix,
//                        the Schedule, koff and the device picture / lambda tables;
//   block k % kOvBlocks  the counters (front end and search); k_front's last workgroup zeroes block
//                        (k + 2) % kOvBlocks.
// and, where the earlier batch ran on another stream (on this stream it precedes in stream order),
//   its front end waits for the search-end event of batch k - 2,
//   its search    waits for the end event of batch k - 2,
//   its tail      waits for the end event of batch k - 1 (the NN state that the tails hand on).
// So the front end of batch k no longer queues behind the tail of batch k - 2: that tail may run
// beside it, as may the tail of batch k - 3 and all of batch k - 1.
//
// Why that is enough.  Search k - 2 was launched behind the end of batch k - 4, and the tails are
// chained, so when the front end of batch k runs, every batch up to k - 4 is over, searches k - 3
// and k - 2 are over, and only the tails of k - 3 and k - 2 and any part of k - 1 may be pending.
//   slot:  perm / cls of slot k % 2 were last read by search k - 2: over.  The records of the slot
//          are written by search k, behind the end of batch k - 2, whose tail read them.
//   ring:  entry k % 4 was last read by the tail of batch k - 4: over.  The tails that may be
//          pending (k - 3, k - 2, k - 1) read the other three entries: four entries are needed.
//   block: a batch uses its block from its front end to the end of its search.  Block k % 4 was
//          used by batch k - 4 and zeroed by front end k - 2, which precedes search k - 2 in stream
//          order: over.  The uses that may overlap batch k's are those of batches k - 1 and k + 1
//          only (front end k + 2 waits for search k), on blocks k - 1 and k + 1.  The block that
//          front end k zeroes, k + 2 = k - 2 (mod 4), was last used by search k - 2 (over) and is
//          next used by front end k + 2 (behind search k, so behind front end k).  Four blocks
//          still do; three would again need an event between consecutive front ends.  A block
//          costs 384 bytes.
//
// A batch with a feature that uses single-buffered context state (kOv* below) waits for every batch
// in flight before anything of it is enqueued, and so does the batch after it: the end events of
// batches k - 1, k - 2 and k - 3 where those ran on other streams (the end of batch k - 1 alone
// implies the others, the tails being chained; the plan names all three so that no reader has to
// follow the chain).  The batch two after a serialised one overlaps again, but its front end waits
// for that batch's end, not for its search: nothing runs beside any part of a serialised batch.
// All waits are stream waits on the earlier batches' events.  The integer
// search is planned like a batch with the feature kOvForeign: it takes a batch number, so its
// counter block comes round zeroed like any other, and it records both events at its end, so the
// batches after it wait for it like for any other.  A batch that the device rejects (an invalid
// job) is committed like any other: its kernels run and skip their work, and its k_front still
// zeroes its block.  Only a batch abandoned on the host after its first launch (a failed launch)
// leaves the blocks in doubt; the next batch then fills them all behind a host-side drain of the
// context.
#pragma once

#include <cstdint>

namespace fme {

constexpr int kOvSlots = 2;
constexpr int kOvRing = 4;
constexpr int kOvBlocks = 4;
constexpr int kOvBack = 3;    // earlier batches that may still be in flight when a batch is planned

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
  int slot = 0;             // work-buffer slot (perm, cls, internal records)
  int block = 0;            // counter block the batch counts in
  int block_zeroed = 0;     // counter block its k_front zeroes
  bool serial = false;      // wait for the end of batches k - 1, k - 2 and k - 3 before anything is enqueued
  bool fill_blocks = false; // the counter blocks are not known to be zero: fill all of them first (serial)
  bool wait_slot = false;   // batch k - 2 ran on another stream.  Serial: before anything, its end.
                            // Otherwise its two events are waited for where wait_front / wait_search say.
  bool wait_prev_front = false;  // serial only: before anything, the end of batch k - 1 (another stream)
  bool wait_prev_tail = false;   // before the tail: the end of batch k - 1 (it ran on another stream)
  int ring = 0;             // ring entry (blk_agg / blk_prefix, Schedule, koff, device tables)
  bool wait_front = false;  // not serial: before k_front, the search-end event of batch k - 2
  bool wait_search = false; // not serial: before the search launch, the end event of batch k - 2
  bool wait_back3 = false;  // serial only: before anything, the end of batch k - 3 (another stream)
  bool wait_front_end = false;   // not serial, batch k - 2 was serialised: before k_front, its end event
                                 // instead of its search-end event (nothing runs beside any part of it)
};

struct OverlapState {
  long long seq = 0;                  // batches enqueued in full
  bool dirty = false;                 // a batch (or integer search) was abandoned half-way
  const void* stream[kOvBack] = {nullptr, nullptr, nullptr};   // of batch seq - 1, seq - 2, seq - 3
  bool live[kOvBack] = {false, false, false};   // there is such a batch (and its two events)
  uint32_t prev_features = 0;         // of batch seq - 1
  uint32_t prev2_features = 0;        // of batch seq - 2
};

inline OverlapPlan overlap_plan(const OverlapState& st, const void* stream, uint32_t features) {
  OverlapPlan p;
  p.slot = (int)(st.seq % kOvSlots);
  p.ring = (int)(st.seq % kOvRing);
  p.block = (int)(st.seq % kOvBlocks);
  p.block_zeroed = (int)((st.seq + 2) % kOvBlocks);
  p.fill_blocks = st.dirty;
  // the batch after a serialised one waits as well: that one may use single-buffered state (the
  // context's staging buffers, the caller's NN bindings) until it ends
  p.serial = features != 0 || st.dirty || st.prev_features != 0;
  const bool other1 = st.live[0] && st.stream[0] != stream;
  const bool other2 = st.live[1] && st.stream[1] != stream;
  const bool other3 = st.live[2] && st.stream[2] != stream;
  // batch k - 2 on this stream is over in stream order; on another stream its events say when
  // (also where batch k - 1, on this stream, has already waited for them: a wait on an event that
  // has fired costs nothing on the device)
  p.wait_slot = other2;
  p.wait_front = other2 && !p.serial && st.prev2_features == 0;
  p.wait_front_end = other2 && !p.serial && st.prev2_features != 0;
  p.wait_search = other2 && !p.serial && !p.wait_front_end;
  p.wait_prev_front = p.serial && other1;
  p.wait_prev_tail = other1 && !p.wait_prev_front;
  p.wait_back3 = p.serial && other3;
  return p;
}

// Before the batch's first launch: whatever happens next, the blocks are in doubt until commit.
inline void overlap_begin(OverlapState& st) { st.dirty = true; }

// Every launch of the batch is enqueued and its events recorded.  A batch that filled the
// counter blocks serialises the next one like a feature: the fill sits on this batch's stream, and
// a batch on another stream that started before it ran would have its block zeroed under it.
inline void overlap_commit(OverlapState& st, const void* stream, uint32_t features, const OverlapPlan& plan) {
  st.seq++;
  st.prev2_features = st.prev_features;
  st.prev_features = features | (plan.fill_blocks ? (uint32_t)kOvFill : 0u);
  st.dirty = false;
  for (int b = kOvBack - 1; b > 0; b--) {
    st.stream[b] = st.stream[b - 1];
    st.live[b] = st.live[b - 1];
  }
  st.stream[0] = stream;
  st.live[0] = true;
}

}  // namespace fme
