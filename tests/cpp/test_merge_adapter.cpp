// GPU test driver of fme_hm::MergeEstimator (include/fme_hm.hpp): a merge fixture exported as raw
// arrays by tests/test_gpu_merge.py, replayed through the adapter and compared record by record.
//
//   test_merge_adapter DIR BIT_DEPTH USE_HADAMARD
//
// DIR holds meta.txt (width height pictures requests lambdas), luma.raw (pictures x height x width
// samples: uint8 at 8 bits, uint16 at 10), lambdas.raw (double), reqs.raw (fme_merge_req),
// res.raw (fme_merge_res).
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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s DIR BIT_DEPTH USE_HADAMARD\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int bit_depth = std::atoi(argv[2]), hadamard = std::atoi(argv[3]);
  int width = 0, height = 0, npic = 0, nreq = 0, nlam = 0;
  {
    FILE* f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d %d %d", &width, &height, &npic, &nreq, &nlam) != 5) {
      std::fprintf(stderr, "bad meta.txt\n");
      return 2;
    }
    std::fclose(f);
  }
  try {
    fme_hm::SearchConfig cfg;
    cfg.useHadamardME = hadamard != 0;
    cfg.nnMode = 0;
    cfg.bitDepth = bit_depth;
    fme_hm::FracSearch search(cfg);
    const size_t plane = (size_t)width * height;
    if (bit_depth > 8) {
      const auto luma = read_raw<uint16_t>(dir + "/luma.raw", plane * npic);
      for (int k = 0; k < npic; k++) search.setPicture16(k, luma.data() + plane * k, width, width, height);
    } else {
      const auto luma = read_raw<uint8_t>(dir + "/luma.raw", plane * npic);
      for (int k = 0; k < npic; k++) search.setPicture8(k, luma.data() + plane * k, width, width, height);
    }
    const auto lambdas = read_raw<double>(dir + "/lambdas.raw", (size_t)nlam);
    for (int k = 0; k < nlam; k++) search.setLambdaSlot(k, lambdas[k]);
    const auto reqs = read_raw<fme_merge_req>(dir + "/reqs.raw", (size_t)nreq);
    const auto want = read_raw<fme_merge_res>(dir + "/res.raw", (size_t)nreq);

    fme_hm::MergeEstimator est(search);
    for (int i = 0; i < nreq; i++)
      if (est.add(reqs[i]) != i) {
        std::fprintf(stderr, "add: index %d\n", i);
        return 1;
      }
    const std::vector<fme_merge_res> got = est.run();
    if ((int)got.size() != nreq || est.pending() != 0) {
      std::fprintf(stderr, "run: %zu results, %d pending\n", got.size(), est.pending());
      return 1;
    }
    int bad = 0;
    for (int i = 0; i < nreq; i++)
      if (std::memcmp(&got[i], &want[i], sizeof(fme_merge_res)) != 0 && bad++ < 5)
        std::fprintf(stderr, "request %d: use_merge %d/%d idx %d/%d merge_cost %u/%u me_cost %u/%u\n", i,
                     got[i].use_merge, want[i].use_merge, got[i].merge_idx, want[i].merge_idx, got[i].merge_cost,
                     want[i].merge_cost, got[i].me_cost, want[i].me_cost);
    if (bad) {
      std::fprintf(stderr, "%d of %d requests differ\n", bad, nreq);
      return 1;
    }
    // an empty queue returns no results; an invalid request throws fme_hm::Error with the library's code
    if (!est.run().empty()) return 1;
    fme_merge_req inv = reqs[0];
    inv.n_cand = 0;
    inv.flags = 0;
    est.add(inv);
    bool threw = false;
    try {
      est.run();
    } catch (const fme_hm::Error& e) {
      threw = e.code() == FME_E_INVALID;
    }
    if (!threw) {
      std::fprintf(stderr, "an invalid request did not throw FME_E_INVALID\n");
      return 1;
    }
    std::printf("merge adapter ok: %d requests at bit depth %d\n", nreq, bit_depth);
  } catch (const fme_hm::Error& e) {
    std::fprintf(stderr, "fme_hm::Error %d: %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
