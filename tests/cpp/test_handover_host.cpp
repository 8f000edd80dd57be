// The hand-over between overlapped batches (csrc/fme_overlap_host.h) on a CPU, from the plans alone.
// A batch is a front end, a search and a tail in stream order; the model knows of no other order
// than the one the plans state: stream order, the waits of a plan (before the front end, before
// the search, before the tail, before everything of a serialised batch) and the host-side drain
// in front of a fill.  Over sequences of 12 batches on streams drawn as k % 1, k % 2, k % 3 and at
// random from three, plain and with a featured batch, an abandoned batch or an integer search
// inserted at each position, it asserts for every pair of batches that
//   - what they share (perm / cls of a slot, the records of a slot, a ring entry, a counter
//     block) is used by one only after the other is done with it, by that order;
//   - no block is zeroed or filled under a batch that counts in it, and every block a batch counts
//     in was zeroed (or filled) after its previous user was done and before the batch starts;
//   - a serialised batch runs beside nothing;
//   - the tails run in batch order (the NN state they hand on).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fme_overlap_host.h"

using namespace fme;

static long long g_cases = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    g_cases++;                                                               \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_what); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)
static char g_what[160] = "";

static const int kStreamIds[3] = {1, 2, 3};
static const void* stream_of(int i) { return &kStreamIds[i]; }

// The six moments of a batch, in stream order.
enum { kFs, kFe, kSs, kSe, kTs, kTe, kMoments };

struct Batch {
  OverlapPlan plan;
  const void* stream = nullptr;
  bool committed = true;   // false: abandoned on the host after its front end's launch
  bool exclusive = false;  // it has a feature or fills the blocks (or was abandoned: its state is unknown)
  int number = -1;         // its batch number (OverlapState::seq when it was planned)
};

struct Model {
  std::vector<Batch> b;
  std::vector<std::vector<bool>> hb;   // hb[x][y]: moment x is over before moment y begins

  int node(int i, int m) const { return i * kMoments + m; }
  // the committed batch with number n, or -1
  int by_number(int n) const {
    for (int i = (int)b.size() - 1; i >= 0; i--)
      if (b[i].committed && b[i].number == n) return i;
    return -1;
  }
  void order(int x, int y) { hb[x][y] = true; }

  void build() {
    const int n = (int)b.size() * kMoments;
    hb.assign(n, std::vector<bool>(n, false));
    for (int j = 0; j < (int)b.size(); j++) {
      const OverlapPlan& p = b[j].plan;
      for (int m = 0; m + 1 < kMoments; m++) order(node(j, m), node(j, m + 1));
      for (int i = j - 1; i >= 0; i--)   // stream order: behind the last batch of this stream
        if (b[i].stream == b[j].stream) {
          order(node(i, kTe), node(j, kFs));
          break;
        }
      const int k1 = by_number(b[j].number - 1), k2 = by_number(b[j].number - 2), k3 = by_number(b[j].number - 3);
      auto earlier = [&](int k) { return k >= 0 && k < j; };
      if (p.serial) {
        if (p.wait_prev_front && earlier(k1)) order(node(k1, kTe), node(j, kFs));
        if (p.wait_slot && earlier(k2)) order(node(k2, kTe), node(j, kFs));
        if (p.wait_back3 && earlier(k3)) order(node(k3, kTe), node(j, kFs));
      } else {
        if (p.wait_front && earlier(k2)) order(node(k2, kSe), node(j, kFs));
        if (p.wait_front_end && earlier(k2)) order(node(k2, kTe), node(j, kFs));
        if (p.wait_search && earlier(k2)) order(node(k2, kTe), node(j, kSs));
      }
      if (p.wait_prev_tail && earlier(k1)) order(node(k1, kTe), node(j, kTs));
      if (p.fill_blocks)   // the host waits for every stream of the context before the fill
        for (int i = 0; i < j; i++) order(node(i, kTe), node(j, kFs));
    }
    for (int k = 0; k < n; k++)
      for (int x = 0; x < n; x++)
        if (hb[x][k])
          for (int y = 0; y < n; y++)
            if (hb[k][y]) hb[x][y] = true;
  }
  bool before(int i, int mi, int j, int mj) const { return hb[node(i, mi)][node(j, mj)]; }
};

static void check_model(Model& m) {
  m.build();
  const int n = (int)m.b.size();
  for (int j = 0; j < n; j++) {
    const OverlapPlan& q = m.b[j].plan;
    for (int i = 0; i < j; i++) {
      const OverlapPlan& p = m.b[i].plan;
      std::snprintf(g_what, sizeof(g_what), "batches %d (number %d) and %d (number %d)", i, m.b[i].number, j, m.b[j].number);
      // an abandoned batch got as far as its front end; the fill behind it orders everything else
      const int i_perm_end = kSe, i_end = kTe;
      if (p.slot == q.slot) {
        CHECK(m.before(i, i_perm_end, j, kFs));   // perm / cls: front end to search
        CHECK(m.before(i, i_end, j, kSs));        // the records: search to tail
      }
      if (p.ring == q.ring) CHECK(m.before(i, i_end, j, kFs));          // front end to tail
      if (p.block == q.block) CHECK(m.before(i, kSe, j, kFs));          // counting: front end to search
      if (q.block_zeroed == p.block) CHECK(m.before(i, kSe, j, kFs));   // j zeroes no block under i
      if (p.block_zeroed == q.block) CHECK(m.before(i, kFe, j, kFs));   // and i none under j
      if (p.fill_blocks) CHECK(m.before(i, kFe, j, kFs));               // a fill touches every block
      if (q.fill_blocks) CHECK(m.before(i, kSe, j, kFs));
      // single-buffered context state: a batch that uses it (a feature, a fill) runs beside nothing,
      // and a serialised batch (one of those, or the batch after one) starts behind everything
      if (m.b[i].exclusive || q.serial) CHECK(m.before(i, kTe, j, kFs));
    }
    if (!m.b[j].committed) continue;
    // the tails in batch order
    const int k1 = m.by_number(m.b[j].number - 1);
    std::snprintf(g_what, sizeof(g_what), "batch %d (number %d)", j, m.b[j].number);
    if (k1 >= 0) CHECK(m.before(k1, kTe, j, kTs));
    // the block it counts in: zeroed or filled since its previous user, and before its front end
    int user = -1;
    for (int i = j - 1; i >= 0 && user < 0; i--)
      if (m.b[i].plan.block == q.block) user = i;
    if (user >= 0 && !q.fill_blocks) {
      bool zeroed = false;
      for (int z = 0; z < j && !zeroed; z++) {
        const OverlapPlan& r = m.b[z].plan;
        if (z == user || !(r.fill_blocks || (r.block_zeroed == q.block && m.b[z].committed))) continue;
        zeroed = m.before(user, kSe, z, kFs) && m.before(z, kFe, j, kFs);
      }
      CHECK(zeroed);
    }
  }
}

enum Special { kNone, kFeatured, kAbandoned, kIntegerSearch };

// 12 batches on streams pick(k); at position `at` the special one.
template <class Pick>
static void run_sequence(Pick pick, Special special, int at) {
  OverlapState st;
  Model m;
  for (int k = 0; k < 12; k++) {
    const void* s = stream_of(pick(k));
    uint32_t feat = 0;
    if (k == at && special == kFeatured) feat = kOvKeys;
    if (k == at && special == kIntegerSearch) feat = kOvForeign;
    if (k == at && special == kAbandoned) {   // planned, first launch enqueued, then a launch fails
      Batch a;
      a.plan = overlap_plan(st, s, 0);
      a.stream = s;
      a.committed = false;
      a.exclusive = true;
      a.number = (int)st.seq;
      overlap_begin(st);
      m.b.push_back(a);
      CHECK(st.dirty);
    }
    Batch b;
    b.plan = overlap_plan(st, s, feat);
    b.stream = s;
    b.number = (int)st.seq;
    b.exclusive = feat != 0 || b.plan.fill_blocks;
    if (k == at && special == kAbandoned) CHECK(b.plan.fill_blocks && b.plan.serial);
    if (feat) CHECK(b.plan.serial);
    CHECK(b.plan.slot == b.number % kOvSlots && b.plan.ring == b.number % kOvRing && b.plan.block == b.number % kOvBlocks);
    CHECK(!(b.plan.serial && (b.plan.wait_front || b.plan.wait_search)));
    overlap_begin(st);
    overlap_commit(st, s, feat, b.plan);
    m.b.push_back(b);
  }
  CHECK(st.seq == 12 && !st.dirty);
  check_model(m);
}

int main() {
  {   // three streams in rotation: the plan of a batch in steady state, spelled out
    OverlapState st;
    for (int k = 0; k < 12; k++) {
      const void* s = stream_of(k % 3);
      const OverlapPlan p = overlap_plan(st, s, 0);
      overlap_begin(st);
      overlap_commit(st, s, 0, p);
      CHECK(!p.serial && !p.fill_blocks && !p.wait_prev_front && !p.wait_back3);
      CHECK(p.wait_front == (k >= 2) && p.wait_search == (k >= 2) && p.wait_prev_tail == (k >= 1));
      CHECK(p.ring == k % 4 && p.slot == k % 2 && p.block == k % 4 && p.block_zeroed == (k + 2) % 4);
    }
  }
  {   // one stream: no waits; two streams: batch k - 2 precedes in stream order
    for (int ns = 1; ns <= 2; ns++) {
      OverlapState st;
      for (int k = 0; k < 12; k++) {
        const void* s = stream_of(k % ns);
        const OverlapPlan p = overlap_plan(st, s, 0);
        overlap_begin(st);
        overlap_commit(st, s, 0, p);
        CHECK(!p.wait_front && !p.wait_search && !p.wait_slot && !p.serial);
        CHECK(p.wait_prev_tail == (ns == 2 && k >= 1));
      }
    }
  }
  {   // a serialised batch on a third stream waits for all three batches in flight
    OverlapState st;
    for (int k = 0; k < 3; k++) {
      const OverlapPlan p = overlap_plan(st, stream_of(k % 2), 0);
      overlap_begin(st);
      overlap_commit(st, stream_of(k % 2), 0, p);
    }
    const OverlapPlan p = overlap_plan(st, stream_of(2), kOvStaged);
    CHECK(p.serial && p.wait_prev_front && p.wait_slot && p.wait_back3 && !p.wait_front && !p.wait_search && !p.wait_prev_tail);
  }
  const Special specials[] = {kNone, kFeatured, kAbandoned, kIntegerSearch};
  for (Special sp : specials) {
    for (int at = 0; at < (sp == kNone ? 1 : 12); at++) {
      for (int ns = 1; ns <= 3; ns++) run_sequence([ns](int k) { return k % ns; }, sp, at);
      for (uint32_t seed = 1; seed <= 8; seed++) {   // random of three
        uint32_t x = seed * 2654435761u;
        int draw[12];
        for (int k = 0; k < 12; k++) {
          x = x * 1664525u + 1013904223u;
          draw[k] = (int)((x >> 16) % 3u);
        }
        run_sequence([&draw](int k) { return draw[k]; }, sp, at);
      }
    }
  }
  std::printf("handover host ok: %lld cases\n", g_cases);
  return 0;
}
