// GPU test driver of fme_hm::CtuRowBatcher and FracSearch::refine with SearchConfig::nnTopK
// (include/fme_hm.hpp): a refinement fixture exported as raw arrays by tests/test_gpu_among.py goes
// through the batcher in rows (uni-pred jobs with add, keyed jobs with addBiPred and their key
// blocks) and is compared byte by byte with the top-K records of the Python path.
//
//   test_topk_adapter DIR BIT_DEPTH USE_HADAMARD FEN QP TOPK
//
// DIR holds meta.txt (width height pictures jobs keys lambdas), pictures.raw (pictures x plane
// samples: uint8 at 8 bits, uint16 at 10), keys.raw (int16), lambdas.raw (double), jobs.raw
// (fme_job), expected.raw (fme_result).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fme_hm.hpp"

namespace {

template <typename T>
std::vector<T> read_raw(const std::string& path, size_t count) {
  std::vector<T> v(count);
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  const size_t got = std::fread(v.data(), sizeof(T), count, f);
  std::fclose(f);
  if (got != count) {
    std::fprintf(stderr, "%s: %zu of %zu records\n", path.c_str(), got, count);
    std::exit(2);
  }
  return v;
}

int compare(const std::vector<fme_result>& got, const std::vector<fme_result>& want, const char* what) {
  int bad = 0;
  for (size_t i = 0; i < want.size(); i++)
    if (std::memcmp(&got[i], &want[i], sizeof(fme_result)) != 0 && bad++ < 5)
      std::fprintf(stderr, "%s job %zu: class %d/%d mv (%d, %d)/(%d, %d) frac_cost %u/%u cost %u/%u bits %u/%u status %x/%x\n",
                   what, i, got[i].nn_class, want[i].nn_class, got[i].mv_x, got[i].mv_y, want[i].mv_x, want[i].mv_y,
                   got[i].frac_cost, want[i].frac_cost, got[i].cost, want[i].cost, got[i].bits, want[i].bits,
                   got[i].status, want[i].status);
  if (bad) std::fprintf(stderr, "%s: %d of %zu jobs differ\n", what, bad, want.size());
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s DIR BIT_DEPTH USE_HADAMARD FEN QP TOPK\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int bit_depth = std::atoi(argv[2]);
  int width = 0, height = 0, npic = 0, njob = 0, nkey = 0, nlam = 0;
  {
    FILE* f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d %d %d %d", &width, &height, &npic, &njob, &nkey, &nlam) != 6) {
      std::fprintf(stderr, "bad meta.txt\n");
      return 2;
    }
    std::fclose(f);
  }
  try {
    fme_hm::SearchConfig cfg;
    cfg.bitDepth = bit_depth;
    cfg.useHadamardME = std::atoi(argv[3]) != 0;
    cfg.fastInterMode = std::atoi(argv[4]);
    cfg.qp = std::atoi(argv[5]);
    cfg.nnDirect = true;
    cfg.nnTopK = std::atoi(argv[6]);
    {   // what the constructor refuses: no nnDirect, k beyond 8, a net the ranking does not know
      struct Case {
        bool direct;
        int mode, k, code;
      };
      const Case cases[] = {{false, 1, 4, FME_E_INVALID}, {true, 1, 9, FME_E_INVALID}, {true, 1, -1, FME_E_INVALID},
                            {true, 2, 4, FME_E_UNSUPPORTED}, {true, 0, 4, FME_E_STATE}};
      for (const Case& q : cases) {
        fme_hm::SearchConfig off = cfg;
        off.nnDirect = q.direct;
        off.nnMode = q.mode;
        off.nnTopK = q.k;
        bool threw = false;
        try {
          fme_hm::FracSearch none(off);
        } catch (const fme_hm::Error& e) {
          threw = e.code() == q.code;
        }
        if (!threw) {
          std::fprintf(stderr, "nnDirect %d nnMode %d nnTopK %d did not throw %d\n", (int)q.direct, q.mode, q.k, q.code);
          return 1;
        }
      }
    }
    fme_hm::FracSearch search(cfg);
    const size_t plane = (size_t)width * height;
    if (bit_depth > 8) {
      const auto pic = read_raw<uint16_t>(dir + "/pictures.raw", plane * npic);
      for (int k = 0; k < npic; k++) search.setPicture16(k, pic.data() + plane * k, width, width, height);
    } else {
      const auto pic = read_raw<uint8_t>(dir + "/pictures.raw", plane * npic);
      for (int k = 0; k < npic; k++) search.setPicture8(k, pic.data() + plane * k, width, width, height);
    }
    const auto lambdas = read_raw<double>(dir + "/lambdas.raw", (size_t)nlam);
    for (int k = 0; k < nlam; k++) search.setLambdaSlot(k, lambdas[k]);
    const auto keys = read_raw<int16_t>(dir + "/keys.raw", (size_t)nkey);
    const auto jobs = read_raw<fme_job>(dir + "/jobs.raw", (size_t)njob);
    const auto want = read_raw<fme_result>(dir + "/expected.raw", (size_t)njob);

    // rows of 97 jobs, two in flight: the NN state follows queue order across the rows
    std::vector<fme_result> got;
    {
      fme_hm::CtuRowBatcher batcher(search);
      std::vector<fme_hm::CtuRowBatcher::Ticket> tickets;
      for (int i = 0; i < njob; i++) {
        if (jobs[i].key_offset >= 0)
          batcher.addBiPred(jobs[i], keys.data() + jobs[i].key_offset, jobs[i].w);
        else
          batcher.add(jobs[i]);
        if (batcher.pending() == 97 || i == njob - 1) tickets.push_back(batcher.submit());
      }
      for (auto t : tickets) {
        const std::vector<fme_result> row = batcher.wait(t);
        got.insert(got.end(), row.begin(), row.end());
      }
    }
    if ((int)got.size() != njob) {
      std::fprintf(stderr, "%zu results of %d\n", got.size(), njob);
      return 1;
    }
    for (int i = 0; i < njob; i++)
      if ((got[i].status & (FME_RES_NN_DIRECT | FME_RES_NN_AMONG | FME_RES_NN_EXTERN)) != (FME_RES_NN_DIRECT | FME_RES_NN_AMONG)) {
        std::fprintf(stderr, "job %d: status %x\n", i, got[i].status);
        return 1;
      }
    if (compare(got, want, "batcher")) return 1;

    // FracSearch::refine: the whole fixture as one batch from a reset state
    if (fme_set_keys(search.ctx(), keys.data(), keys.size(), nullptr) != FME_OK || fme_nn_reset_state(search.ctx()) != FME_OK) {
      std::fprintf(stderr, "%s\n", fme_last_error());
      return 1;
    }
    std::vector<fme_result> one((size_t)njob);
    search.refine(jobs.data(), one.data(), njob);
    if (compare(one, want, "refine")) return 1;
    // an invalid job throws fme_hm::Error with the library's code
    std::vector<fme_job> inv(jobs.begin(), jobs.begin() + 8);
    inv[3].w = 6;
    bool threw = false;
    try {
      search.refine(inv.data(), one.data(), 8);
    } catch (const fme_hm::Error& e) {
      threw = e.code() == FME_E_INVALID;
    }
    if (!threw) {
      std::fprintf(stderr, "an invalid job did not throw FME_E_INVALID\n");
      return 1;
    }
    std::printf("topk adapter ok: %d jobs at bit depth %d, k = %d\n", njob, bit_depth, cfg.nnTopK);
  } catch (const fme_hm::Error& e) {
    std::fprintf(stderr, "fme_hm::Error %d: %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
