// fme_extern.hip — the two kernels of the external-predictor path (include/fme_extern.h) on gfx950,
// one source for 8 and 10 bits.  fme_nn_inputs* is k_front, k_direct_emi (fme_direct.hip) on
// context-internal records, then k_nn_rows; fme_refine_at* is k_front, k_direct_emi unless the
// caller brings rows, then the evaluation (inputs_batch, at_batch, fme_api.cpp).
//
// k_nn_rows: one lane per job, one wave per workgroup, the last-writer scan over the wave and
// backwards through its scan block (writer_scan_wave, with k_front's blk_prefix as the carry-in),
// then the carried-input rule, which fme_device.h states once for this kernel and for the NN tail
// (nn_carried, nn_carried_status, nn_carry_on; k_nn_deep_tail is the one deliberate exception and
// keeps its own statement).  What tail_job hands to nn_forward goes into the job's row, as four
// 16-byte stores, and the last job writes the state.  Unlike the tail it does so in every nn_mode.
//
// The evaluation: k_direct_eval<k10, ExternArgs> (fme_direct_eval.h), the direct batch's kernel with
// the class read from the caller's array, jobs refused one by one, and the record's EMI fields
// taken from the row when there is one.
#include <hip/hip_runtime.h>

#include "fme_device.h"
#include "fme_direct_eval.h"
#include "fme_extern_host.h"

namespace fme {
namespace {

using namespace di;

constexpr int kRowsNT = 64;

__global__ __launch_bounds__(kRowsNT) void k_nn_rows(BatchArgs a, WorkBufs w, fme_nn_row* rows, int state_in,
                                                     int slot_reset) {
  const int wbase = (int)blockIdx.x * kRowsNT;   // the wave's first job (< a.n by the grid)
  const int i = wbase + (int)threadIdx.x;
  const bool valid = i < a.n;
  const uint32_t* st_in = w.nn_state + 12 * state_in;
  uint32_t* st_out = w.nn_state + 12 * (state_in ^ 1);
  if (w.sched->invalid) {   // a rejected batch: the rows marked, the state carried through
    if (valid) {
      g_di_u4* o = (g_di_u4*)(rows + i);
      const di_u4 z{0u, 0u, 0u, 0u};
      o[0] = z;
      o[1] = z;
      o[2] = z;
      o[3] = di_u4{(uint32_t)FME_RES_REJECTED << 16, 0u, 0u, 0u};
      if (i == 0)
        for (int k = 0; k < 12; k++) st_out[k] = st_in[k];
    }
    return;
  }
  fme_job j{};
  di_u4 r0{}, r1{}, r2{}, r3{};   // the job's record as k_direct_emi left it
  if (valid) {
    j = load_job(a, i);
    const fme_result* rec = search_rec(a, w, i);
    r0 = di_ld16(rec, 0);
    r1 = di_ld16(rec, 1);
    r2 = di_ld16(rec, 2);
    r3 = di_ld16(rec, 3);
  }
  // writer indices of this job (slots it pushes, C / PU size)
  int run[9];
  const bool wr = valid && nn_writes_c(j);
  {
    const int np = wr ? nn_pushes(j) : 0;
#pragma unroll
    for (int s = 0; s < 8; s++) run[s] = (np > s) ? i : -1;
    run[8] = wr ? i : -1;
  }
  int src[9];
  writer_scan_wave(a, run, w.blk_prefix + (wbase / kJobsPerScanBlock) * 9, wbase, src);
  if (!valid) return;
  const uint32_t own_emi[8] = {r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z};
  const uint32_t own_c = r1.z, own_n_emi = r3.w & 0xFFu;
  NnCarried v;
  nn_carried(a, w, st_in, i, j, src, own_emi, own_c, slot_reset != 0, v);
  const uint32_t status = nn_carried_status(wr, own_n_emi, v);
  g_di_u4* o = (g_di_u4*)(rows + i);
  o[0] = di_u4{v.e[0], v.e[1], v.e[2], v.e[3]};
  o[1] = di_u4{v.e[4], v.e[5], v.e[6], v.e[7]};
  o[2] = di_u4{v.c, v.ph, v.pw, r0.x};   // r0.x: mv_int_x, mv_int_y
  o[3] = di_u4{own_n_emi | (wr ? 0x100u : 0u) | (status << 16), 0u, 0u, 0u};
  if (i == a.n - 1) nn_carry_on(st_out, v);
}

}  // namespace

static_assert(sizeof(fme_nn_row) == 64 && offsetof(fme_nn_row, c) == 32 && offsetof(fme_nn_row, mv_int_x) == 44 &&
                  offsetof(fme_nn_row, n_emi) == 48 && offsetof(fme_nn_row, writes) == 49 &&
                  offsetof(fme_nn_row, status) == 50 && offsetof(fme_nn_row, reserved) == 52,
              "fme_nn_row layout (k_nn_rows stores it as words)");

hipError_t launch_nn_rows(const BatchArgs& a, const WorkBufs& w, fme_nn_row* rows, int state_in, bool slot_reset,
                          hipStream_t s) {
  if (a.n > 0)
    hipLaunchKernelGGL(k_nn_rows, dim3((a.n + kRowsNT - 1) / kRowsNT), dim3(kRowsNT), 0, s, a, w, rows, state_in,
                       slot_reset ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_at_eval(const ExternArgs& x, hipStream_t s) {
  return launch_by_depth(k_direct_eval<false, ExternArgs>, k_direct_eval<true, ExternArgs>, (x.n + kDiTasks - 1) / kDiTasks, kDiBlock, x, s);
}

}  // namespace fme
