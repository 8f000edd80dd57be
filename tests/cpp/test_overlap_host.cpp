// The batch overlap planner (csrc/fme_overlap_host.h) alone, on a CPU: slot and counter-block
// rotation, the waits on one stream, on alternating streams and after a stream change, every
// serialising feature (the integer search among them), a batch the device rejects, and a batch
// abandoned half-way with the fill of the counter blocks that follows it.  Besides the case
// checks, a model of the device: every plan is replayed against the set of batches that may still
// run, and no batch may touch a slot or a counter block that such a batch uses; a batch that fills
// the counter blocks touches every block.
//
// A batch that the device rejects (an invalid job) is nothing special to the planner: the host
// does not know of it when it plans the next batch, every kernel of it is launched and skips its
// work, and its k_front still zeroes the block it is due to zero.  It is committed like any other
// batch, which the "rejected" case below spells out.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fme_overlap_host.h"

using namespace fme;

static int g_cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_cases++;                                                             \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static const int kStreamA = 1, kStreamB = 2, kStreamC = 3;
static const void* A = &kStreamA;
static const void* B = &kStreamB;
static const void* C = &kStreamC;

static OverlapPlan issue(OverlapState& st, const void* s, uint32_t features = 0) {
  const OverlapPlan p = overlap_plan(st, s, features);
  overlap_begin(st);
  overlap_commit(st, s, features, p);
  return p;
}

// Model: batch k is known to be over before batch j's k_front when j's stream waited for its end
// (directly, or through a batch that follows k in the chain of waits), or when k precedes j on j's
// stream.  over[j][k] for k < j.
struct Model {
  std::vector<const void*> stream;
  std::vector<OverlapPlan> plan;
  std::vector<std::vector<bool>> over_front, over_end;   // before j's k_front / at j's end: batch k is over
  void add(const void* s, const OverlapPlan& p) {
    const int j = (int)stream.size();
    std::vector<bool> f(j, false);
    auto absorb = [&](std::vector<bool>& dst, int k) {   // k is over, and so is all that was over at k's end
      dst[k] = true;
      for (int q = 0; q < k; q++)
        if (over_end[k][q]) dst[q] = true;
    };
    for (int k = j - 1; k >= 0; k--)
      if (stream[k] == s) {
        absorb(f, k);
        break;
      }
    if (p.wait_slot && j >= 2) absorb(f, j - 2);
    if (p.wait_prev_front && j >= 1) absorb(f, j - 1);
    std::vector<bool> e = f;
    if (p.wait_prev_tail && j >= 1) absorb(e, j - 1);
    for (int k = j - 1; k >= 0; k--)   // the tails are ordered: the previous batch's tail is over at j's end
      if (k == j - 1 && (stream[k] == s || p.wait_prev_tail || p.wait_prev_front)) absorb(e, k);
    stream.push_back(s);
    plan.push_back(p);
    over_front.push_back(f);
    over_end.push_back(e);
  }
};

static void check_model(const Model& m) {
  const int n = (int)m.stream.size();
  for (int j = 0; j < n; j++) {
    const OverlapPlan& p = m.plan[j];
    CHECK(j == 0 || m.over_end[j][j - 1]);   // the NN state: tail j runs after tail j - 1
    for (int k = 0; k < j; k++) {
      if (m.over_front[j][k]) continue;
      const OverlapPlan& q = m.plan[k];      // batch k may still run while batch j does
      CHECK(!p.serial);
      CHECK(q.slot != p.slot);
      CHECK(q.block != p.block);             // counting, tile queues
      CHECK(q.block != p.block_zeroed);      // j zeroes no block that k uses
      CHECK(q.block_zeroed != p.block);      // and k none that j uses
      CHECK(!p.fill_blocks && !q.fill_blocks);   // a fill touches every block: nothing runs beside it
    }
    // the block j counts in was zeroed by a batch whose k_front is over, and not used since
    if (j >= 2) {
      CHECK(m.plan[j - 2].block_zeroed == p.block && m.over_front[j][j - 2]);
      CHECK(m.plan[j - 1].block != p.block);
    }
  }
}

int main() {
  {   // rotation, one stream: no waits at all
    OverlapState st;
    for (int k = 0; k < 12; k++) {
      const OverlapPlan p = issue(st, A);
      CHECK(p.slot == k % 2 && p.block == k % kOvBlocks && p.block_zeroed == (k + 2) % kOvBlocks);
      CHECK(!p.serial && !p.fill_blocks && !p.wait_slot && !p.wait_prev_front && !p.wait_prev_tail);
    }
    CHECK(st.seq == 12);
  }
  {   // alternating streams: the tail waits for the previous batch, nothing else (batch k - 2 is on this stream)
    OverlapState st;
    Model m;
    for (int k = 0; k < 12; k++) {
      const void* s = k % 2 ? B : A;
      const OverlapPlan p = issue(st, s);
      m.add(s, p);
      CHECK(p.slot == k % 2 && p.block == k % kOvBlocks);
      CHECK(!p.serial && !p.wait_slot && !p.wait_prev_front);
      CHECK(p.wait_prev_tail == (k >= 1));
    }
    check_model(m);
  }
  {   // stream changes: A A B B A C C A ...
    const void* seq[] = {A, A, B, B, A, C, C, A, B, C, A, A, C, B, B, B, A};
    OverlapState st;
    Model m;
    const void* prev = nullptr;
    const void* prev2 = nullptr;
    int k = 0;
    for (const void* s : seq) {
      const OverlapPlan p = issue(st, s);
      m.add(s, p);
      CHECK(!p.serial);
      CHECK(p.wait_slot == (k >= 2 && prev2 != s));
      CHECK(p.wait_prev_tail == (k >= 1 && prev != s));
      prev2 = prev;
      prev = s;
      k++;
    }
    check_model(m);
  }
  {   // every feature serialises the batch and the one after it, on either stream
    const uint32_t feats[] = {kOvKeys, kOvDeepNn, kOvPx, kOvStaged, kOvGrow, kOvForeign, kOvKeys | kOvGrow};
    for (uint32_t f : feats) {
      OverlapState st;
      Model m;
      m.add(A, issue(st, A));
      m.add(B, issue(st, B));
      const OverlapPlan p = issue(st, A, f);   // batch 2: batch 1 (B) may run, batch 0 (A) precedes it
      m.add(A, p);
      CHECK(p.serial && p.wait_prev_front && !p.wait_prev_tail && !p.wait_slot && !p.fill_blocks);
      CHECK(p.slot == 0 && p.block == 2);
      const OverlapPlan q = issue(st, B);      // the batch after it waits for it as well
      m.add(B, q);
      CHECK(q.serial && q.wait_prev_front && !q.wait_prev_tail);
      const OverlapPlan r = issue(st, A);      // and the next one overlaps again
      m.add(A, r);
      CHECK(!r.serial && r.wait_prev_tail && !r.wait_prev_front);
      const OverlapPlan t = issue(st, C, f);   // a third stream: both batches in flight are waited for
      m.add(C, t);
      CHECK(t.serial && t.wait_prev_front && t.wait_slot);
      check_model(m);
    }
  }
  {   // a batch abandoned after its first launch: the next one fills the blocks behind everything
    OverlapState st;
    issue(st, A);
    issue(st, B);
    const OverlapPlan p = overlap_plan(st, A, 0);
    overlap_begin(st);                        // ... and a launch fails: no commit
    CHECK(st.dirty && st.seq == 2);
    const OverlapPlan q = overlap_plan(st, A, 0);
    CHECK(q.slot == p.slot && q.block == p.block);   // the same batch number again
    CHECK(q.fill_blocks && q.serial && q.wait_prev_front);
    overlap_begin(st);
    overlap_commit(st, A, 0, q);
    CHECK(!st.dirty && st.seq == 3);
    // the fill sits on A: the next batch, on B, must not start before it has run
    const OverlapPlan r = issue(st, B);
    CHECK(!r.fill_blocks && r.serial && r.wait_prev_front && !r.wait_prev_tail);
    const OverlapPlan t = issue(st, A);
    CHECK(!t.fill_blocks && !t.serial && t.wait_prev_tail);
  }
  {   // the same through the model: fill on either stream, the batches after it on the other
    for (int v = 0; v < 2; v++) {
      OverlapState st;
      Model m;
      m.add(A, issue(st, A));
      m.add(B, issue(st, B));
      overlap_begin(st);   // abandoned
      const void* s0 = v ? A : B;
      const void* s1 = v ? B : A;
      for (int k = 0; k < 6; k++) {
        const void* s = k % 2 ? s1 : s0;
        const OverlapPlan p = issue(st, s);
        CHECK(p.fill_blocks == (k == 0));
        m.add(s, p);
      }
      check_model(m);
    }
  }
  {   // rejected on the device: planned and committed like any batch, the rotation goes on
    OverlapState st;
    Model m;
    for (int k = 0; k < 8; k++) {
      const void* s = k % 2 ? B : A;
      const OverlapPlan p = issue(st, s);   // k == 3 is the rejected one: nothing differs
      m.add(s, p);
      CHECK(p.slot == k % 2 && p.block == k % kOvBlocks && p.block_zeroed == (k + 2) % kOvBlocks);
      CHECK(!p.serial && !p.fill_blocks && !st.dirty);
    }
    check_model(m);
  }
  {   // the integer search between overlapped batches, on either stream: it and the batch after it are serial
    for (int v = 0; v < 2; v++) {
      OverlapState st;
      Model m;
      m.add(A, issue(st, A));
      m.add(B, issue(st, B));
      const void* sz = v ? A : B;
      const OverlapPlan z = issue(st, sz, kOvForeign);
      m.add(sz, z);
      CHECK(z.serial && !z.fill_blocks && z.block == 2 && z.block_zeroed == 0);
      const OverlapPlan p = issue(st, v ? B : A);   // on the other stream: waits for the search's end
      m.add(v ? B : A, p);
      CHECK(p.serial && p.wait_prev_front && !p.fill_blocks && p.block == 3);
      const OverlapPlan q = issue(st, sz);
      m.add(sz, q);
      CHECK(!q.serial && q.wait_prev_tail && q.block == 0);   // zeroed by the search's scatter
      m.add(v ? B : A, issue(st, v ? B : A));
      check_model(m);
    }
  }
  {   // the first batches: nothing to wait for
    OverlapState st;
    const OverlapPlan p = issue(st, B, kOvGrow);
    CHECK(p.serial && !p.wait_prev_front && !p.wait_slot && !p.wait_prev_tail);
  }
  std::printf("overlap host ok: %d cases\n", g_cases);
  return 0;
}
