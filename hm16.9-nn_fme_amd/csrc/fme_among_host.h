// fme_among_host.h — the arithmetic of candidate-set refinement (include/fme_among.h) that needs no
// GPU: which slot values are classes, which lists refuse their job, the pick over a list's costs
// (the first least, empties skipped), the insertion that keeps the k best (value, class) pairs, and
// the argument checks of the entry points.  Plain C++ over include/fme_among.h: no HIP, so a CPU test
// can include it alone (tests/cpp/test_among_host.cpp); the kernels (fme_among.hip) and the runtime
// include it too, hence FME_EXTERN_HD.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/fme_among.h"
#include "fme_extern_host.h"

namespace fme {

static_assert((FME_RES_NN_AMONG & (FME_RES_NN_STALE | FME_RES_NN_UNINIT | FME_RES_NN_DIRECT | FME_RES_NN_EXTERN |
                                   FME_RES_REJECTED)) == 0,
              "FME_RES_NN_AMONG is a status bit of its own");
static_assert(FME_AMONG_MAX == 8, "a job's list is one 8-byte word, its costs one 8-word LDS row");

constexpr uint32_t kAmongNone = 0xFFFFFFFFu;   // the cost word of an empty slot / a refused job

FME_EXTERN_HD bool among_k_ok(int k) { return k >= 1 && k <= FME_AMONG_MAX; }
FME_EXTERN_HD bool among_slot_empty(int v) { return v == (int)FME_AMONG_EMPTY; }
// A slot value a list may hold: a class or the empty mark.
FME_EXTERN_HD bool among_slot_ok(int v) { return among_slot_empty(v) || extern_class_ok(v); }

// A list the evaluation accepts: every slot a class or empty, and at least one class.
FME_EXTERN_HD bool among_list_ok(const uint8_t* slots, int k) {
  bool any = false;
  for (int s = 0; s < k; s++) {
    if (!among_slot_ok(slots[s])) return false;
    any = any || !among_slot_empty(slots[s]);
  }
  return any;
}

// The chosen slot of an accepted list: the first of least cost among the non-empty ones (strict <,
// in slot order); -1 when every slot is empty.
FME_EXTERN_HD int among_pick(const uint8_t* slots, const uint32_t* cost, int k) {
  int best = -1;
  for (int s = 0; s < k; s++)
    if (!among_slot_empty(slots[s]) && (best < 0 || cost[s] < cost[best])) best = s;
  return best;
}

// The k best (value, class) pairs seen so far, best first; filled: how many are held (<= k).  A new
// pair goes in front of the first held value it beats (strict >), so equal values keep the order
// they came in: with the classes offered in index order, the lower class first.
template <class T>
FME_EXTERN_HD void among_insert(T* val, uint8_t* cls, int k, int& filled, T v, int c) {
  int p = filled;
  while (p > 0 && v > val[p - 1]) p--;
  if (p >= k) return;
  const int last = filled < k ? filled : k - 1;
  for (int q = last; q > p; q--) {
    val[q] = val[q - 1];
    cls[q] = cls[q - 1];
  }
  val[p] = v;
  cls[p] = (uint8_t)c;
  if (filled < k) filled++;
}

// The entry points' argument checks: 0 (run), 1 (n == 0: nothing to do) or a negative FME_E_* code.
// bound: NN input rows are bound to the context (fme_set_nn_inputs).
inline int among_request(const void* ctx, const void* jobs, const void* cand, int k, const void* out, int n, bool bound) {
  if (!ctx || n < 0 || !among_k_ok(k) || (n > 0 && (!jobs || !cand || !out))) return FME_E_INVALID;
  if (bound) return FME_E_STATE;
  return n == 0 ? 1 : 0;
}
// nn_mode: the context's; loaded: the two-layer net's weights are.
inline int among_net_state(int nn_mode, bool loaded) {
  if (nn_mode == 2) return FME_E_UNSUPPORTED;
  if (nn_mode != 1 || !loaded) return FME_E_STATE;
  return 0;
}
inline int among_rank_request(const void* ctx, const void* rows, const void* cand, int k, int n, int nn_mode,
                              bool loaded) {
  if (!ctx || n < 0 || !among_k_ok(k) || (n > 0 && (!rows || !cand))) return FME_E_INVALID;
  const int st = among_net_state(nn_mode, loaded);
  if (st) return st;
  return n == 0 ? 1 : 0;
}
inline int among_topk_request(const void* ctx, const void* jobs, const void* out, int k, int n, bool bound, int nn_mode,
                              bool loaded) {
  if (!ctx || n < 0 || !among_k_ok(k) || (n > 0 && (!jobs || !out))) return FME_E_INVALID;
  if (bound) return FME_E_STATE;
  const int st = among_net_state(nn_mode, loaded);
  if (st) return st;
  return n == 0 ? 1 : 0;
}

// The host-array form's check before anything is enqueued: the first job a batch would refuse, or -1.
inline int among_first_refused(const fme_job* jobs, const fme_nn_row* rows, const uint8_t* cand, int k, int n) {
  for (int i = 0; i < n; i++) {
    if (!among_list_ok(cand + (size_t)i * k, k)) return i;
    if (rows && !extern_row_ok(rows[i], jobs[i].mv_x, jobs[i].mv_y)) return i;
  }
  return -1;
}

}  // namespace fme
