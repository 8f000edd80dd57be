// fme_pi_host.h — the predInterSearch producers' host arithmetic (fme_producers.cpp): HM's bit
// counts and cost tails, and the steps the P and B producers share, each defined once: the search
// job of one (PU, reference), the AMVP choice, the m_integerMv2Nx2N dependency levels and their
// launch order.  Plain C++ over include/fme.h: no HIP, so a CPU test can include it alone
// (tests/cpp/test_pi_host.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fme.h"

namespace fme {

// xGetMvpIdxBits (TEncSearch.cpp:4258-4284); m_auiMVPIdxCost[idx][num] (412-425)
inline uint32_t mvp_idx_bits(int idx, int num) {
  if (num == 1) return 0;
  if (idx == 0) return 1;
  return 1u + (uint32_t)(idx - 1) + (num - 1 > idx ? 1u : 0u);
}
// xGetBlkBits (TEncSearch.cpp:4286-4333), P slice: uiBlkBit[0]
inline uint32_t blk_bits_p(int part_size) {
  return (part_size == FME_PART_2Nx2N || part_size == FME_PART_NxN) ? 1u : 3u;
}
// TComRdCost::xGetExpGolombNumberOfBits (TComRdCost.cpp:172-185)
inline uint32_t eg_bits(int v) {
  uint32_t t = v <= 0 ? ((uint32_t)(-v) << 1) + 1u : (uint32_t)v << 1;
  uint32_t len = 1;
  while (t != 1) {
    t >>= 1;
    len += 2;
  }
  return len;
}
// TComRdCost::getCost (TComRdCost.h:165)
inline uint32_t rd_cost(double ml, uint32_t bits) { return (uint32_t)((ml * (double)bits) / 65536.0); }
// TComDataCU::clipMv (TComDataCU.cpp:2773-2786), max CU 64, quarter-pel
inline void clip_qpel(int& x, int& y, int pw, int ph, int cu_x, int cu_y) {
  x = std::min((pw + 8 - cu_x - 1) << 2, std::max((-64 - 8 - cu_x + 1) * 4, x));
  y = std::min((ph + 8 - cu_y - 1) << 2, std::max((-64 - 8 - cu_y + 1) * 4, y));
}
inline int round4(int v) { return (v + 2) >> 2; }   // TComMv::divideByPowerOf2(2)

// xGetBlkBits (TEncSearch.cpp:4286-4333), B slice: uiBlkBit[0..2]
inline void blk_bits_b(int part_size, int part_idx, int last_mode, uint32_t out[3]) {
  static const uint32_t hor[2][3][3] = {{{0, 0, 3}, {0, 0, 0}, {0, 0, 0}}, {{5, 7, 7}, {7, 5, 7}, {6, 6, 6}}};
  static const uint32_t ver[2][3][3] = {{{0, 2, 3}, {0, 0, 0}, {0, 0, 0}}, {{5, 7, 7}, {5, 5, 7}, {6, 6, 6}}};
  if (part_size == FME_PART_2Nx2N || part_size == FME_PART_NxN) {
    out[0] = 3; out[1] = 3; out[2] = 5;
    return;
  }
  const bool hz = part_size == FME_PART_2NxN || part_size == FME_PART_2NxnU || part_size == FME_PART_2NxnD;
  const uint32_t* t = hz ? hor[part_idx][last_mode] : ver[part_idx][last_mode];
  out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
}
inline uint32_t ref_bits(int k, int num_refs) {   // TEncSearch.cpp:3792-3800
  return num_refs <= 1 ? 0u : (uint32_t)k + 1u - (k == num_refs - 1 ? 1u : 0u);
}
// xCheckBestMVP (TEncSearch.cpp:4344-4394), cost scale 0
inline void check_best_mvp(double ml, const int16_t cand[2][2], int n_cand, int mx, int my, int& idx, uint32_t& bits,
                           uint32_t& cost) {
  if (n_cand < 2) return;
  const int org_bits = (int)(eg_bits(mx - cand[idx][0]) + eg_bits(my - cand[idx][1]) + mvp_idx_bits(idx, 2));
  int best_bits = org_bits, best_idx = idx;
  for (int m = 0; m < n_cand; m++) {
    if (m == idx) continue;
    const int b = (int)(eg_bits(mx - cand[m][0]) + eg_bits(my - cand[m][1]) + mvp_idx_bits(m, 2));
    if (b < best_bits) {
      best_bits = b;
      best_idx = m;
    }
  }
  if (best_idx != idx) {
    idx = best_idx;
    const uint32_t org_total = bits;
    bits = org_total - (uint32_t)org_bits + (uint32_t)best_bits;
    cost = (cost - rd_cost(ml, org_total)) + rd_cost(ml, bits);
  }
}
// xMotionEstimation's cost tail (TEncSearch.cpp:4594-4597) re-priced for bits_in + extra bits: the
// searches do not read bits_in, so a job run with a provisional bits_in gives the exact result.
inline uint32_t tail_cost(double ml, const fme_result& r, uint32_t bits_in, uint32_t extra, double fw) {
  const uint32_t mvb = r.bits - bits_in;
  const double v = floor(fw * ((double)r.frac_cost - (double)rd_cost(ml, mvb))) + (double)rd_cost(ml, r.bits + extra);
  return (uint32_t)(int64_t)v;
}

inline int two_part(int part_size) { return part_size != FME_PART_2Nx2N && part_size != FME_PART_NxN; }
inline int num_parts(int part_size) { return part_size == FME_PART_2Nx2N ? 1 : (part_size == FME_PART_NxN ? 4 : 2); }

// One xMotionEstimation call as a search job and its fme_tz_ext: request q (fme_pu_req or
// fme_pu_req_b) on reference slot ref_id, predictor pred, xSetSearchRange (TEncSearch.cpp:4602-4624)
// of +-range full-pel around the quarter-pel centre (cx, cy).  job_flags: FME_JOB_EMI or
// FME_JOB_BIPRED (the request's lossless flag is added here); pred2n: the job reads
// m_integerMv2Nx2N (the caller fills pred2n_x / pred2n_y).  Every other field is zero.
template <typename Req>
inline void search_job(const Req& q, int pic_w, int pic_h, uint8_t ref_id, const int16_t pred[2], int cx, int cy,
                       int range, uint32_t job_flags, uint32_t bits_in, int32_t key_offset, bool pred2n, fme_job& j,
                       fme_tz_ext& e) {
  clip_qpel(cx, cy, pic_w, pic_h, q.cu_x, q.cu_y);
  int lx = cx - (range << 2), ly = cy - (range << 2), rx = cx + (range << 2), ry = cy + (range << 2);
  clip_qpel(lx, ly, pic_w, pic_h, q.cu_x, q.cu_y);
  clip_qpel(rx, ry, pic_w, pic_h, q.cu_x, q.cu_y);
  j = fme_job{};
  j.x = q.x; j.y = q.y; j.w = q.w; j.h = q.h;
  j.org_id = q.org_id; j.ref_id = ref_id;
  j.mvp_x = pred[0]; j.mvp_y = pred[1];
  j.lt_x = (int16_t)round4(lx); j.lt_y = (int16_t)round4(ly);
  j.rb_x = (int16_t)round4(rx); j.rb_y = (int16_t)round4(ry);
  j.flags = (uint8_t)(job_flags | ((q.flags & FME_PU_LOSSLESS) ? FME_JOB_LOSSLESS : 0u));
  j.lambda_id = q.lambda_id;
  j.bits_in = (uint16_t)bits_in;
  j.key_offset = key_offset;
  e = fme_tz_ext{};
  e.cu_x = q.cu_x; e.cu_y = q.cu_y;
  e.search_range = (uint8_t)range;
  e.flags = pred2n ? FME_TZ_PRED2NX2N : 0;
}

// xGetTemplateCost's calcRdCost(bits, SAD, DF_SAD) with bits = m_auiMVPIdxCost[m][AMVP_MAX_NUM_CANDS]
// (TEncSearch.cpp:4423-4433)
inline uint32_t template_cost(uint32_t sad, int m, double ml) {
  return (uint32_t)((double)sad + ((double)mvp_idx_bits(m, 2) * ml) / 65536.0);
}
// xEstimateMvPredAMVP's choice over the nc template SADs of one (PU, reference): uiBestCost >
// uiTmpCost, so the first least cost wins.  Returns the index; best: its cost.
inline int amvp_pick(const uint32_t* sad, int nc, double ml, uint32_t& best) {
  int idx = 0;
  best = 0xFFFFFFFFu;
  for (int m = 0; m < nc; m++) {
    const uint32_t cost = template_cost(sad[m], m, ml);
    if (best > cost) {
      best = cost;
      idx = m;
    }
  }
  return idx;
}

// A request reads m_integerMv2Nx2N unless it is the 2Nx2N PU of a depth-0 CU; a 2Nx2N request writes it.
template <typename Req>
inline bool reads_2n(const Req& q) { return !(q.part_size == FME_PART_2Nx2N && q.depth == 0); }

// The m_integerMv2Nx2N dependency levels of requests reqs[0..n) in call order.  Request i owns jobs
// beg[i] .. beg[i+1]-1; key_of(i, u) is its job u's (list, reference) slot l * 4 + k.  A reader waits
// for the latest earlier 2Nx2N job on its slot: src[u] is that job (-1: none, and ext[u].pred2n_*
// get the carried table's value), lvl[u] the level of u's request, one above the highest level among
// its sources.  last[slot]: the last writing job (-1: none).  Returns the highest level.
template <typename Req, typename KeyOf>
inline int assign_levels(const Req* reqs, int n, const int* beg, KeyOf key_of, const int16_t carried[2][FME_MAX_REFS][2],
                         fme_tz_ext* ext, int* src, int* lvl, int last[2 * FME_MAX_REFS]) {
  int last_lvl[2 * FME_MAX_REFS];   // the level of last[slot]
  for (int k = 0; k < 2 * FME_MAX_REFS; k++) last[k] = last_lvl[k] = -1;
  std::fill(src, src + beg[n], -1);   // one streaming fill; the loop writes only the readers' sources
  int max_level = 0;
  for (int i = 0; i < n; i++) {
    const int b = beg[i], e = beg[i + 1];
    const bool rd = reads_2n(reqs[i]);
    int level = 0;
    if (rd)
      for (int u = b; u < e; u++) level = std::max(level, last_lvl[key_of(i, u)] + 1);
    max_level = std::max(max_level, level);
    for (int u = b; u < e; u++) {
      lvl[u] = level;
      if (!rd) continue;
      const int key = key_of(i, u);
      if (last[key] >= 0) {
        src[u] = last[key];
      } else {
        ext[u].pred2n_x = carried[key >> 2][key & 3][0];
        ext[u].pred2n_y = carried[key >> 2][key & 3][1];
      }
    }
    if (reqs[i].part_size == FME_PART_2Nx2N)
      for (int u = b; u < e; u++) {
        last[key_of(i, u)] = u;
        last_lvl[key_of(i, u)] = level;
      }
  }
  return max_level;
}

// The launch order of the levels (k_tz_level): jobs sorted by level, within a level the largest
// PUs first (blocks dispatch in index order, so the longest searches of a wide level start at once
// instead of forming its tail).  off[l] .. off[l+1]: the positions of level l; order[q]: the job at
// position q; pos: its inverse.  off, fill, start and byarea are the caller's kept scratch.
inline void level_order(const fme_job* jobs, const int* lvl, int nj, int max_level, std::vector<int32_t>& off,
                        std::vector<int32_t>& fill, std::vector<int>& start, std::vector<int>& byarea, int32_t* order,
                        int32_t* pos) {
  off.assign((size_t)max_level + 2, 0);
  for (int u = 0; u < nj; u++) off[lvl[u] + 1]++;
  for (int l = 0; l <= max_level; l++) off[l + 1] += off[l];
  fill.assign(off.begin(), off.end() - 1);
  start.assign(64 * 64 + 2, 0);   // counting sort by area, descending
  for (int u = 0; u < nj; u++) start[64 * 64 - (int)jobs[u].w * jobs[u].h + 1]++;
  for (size_t a = 1; a < start.size(); a++) start[a] += start[a - 1];
  byarea.resize((size_t)nj);
  for (int u = 0; u < nj; u++) byarea[start[64 * 64 - (int)jobs[u].w * jobs[u].h]++] = u;
  for (int u : byarea) {
    pos[u] = fill[lvl[u]]++;
    order[pos[u]] = u;
  }
}
// psrc[q] for the positions lo .. hi-1 (a range, so that the caller can thread it): the position of
// the source of the job at q, or -1
inline void level_psrc(const int* src, const int32_t* order, const int32_t* pos, int lo, int hi, int32_t* psrc) {
  for (int q = lo; q < hi; q++) psrc[q] = src[order[q]] >= 0 ? pos[src[order[q]]] : -1;
}

}  // namespace fme
