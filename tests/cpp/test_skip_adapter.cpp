// GPU test driver of fme_hm::SkipEstimator (include/fme_hm.hpp): a skip fixture exported as raw
// arrays by tests/test_gpu_skip.py, replayed through the adapter slice by slice and compared record
// by record.
//
//   test_skip_adapter DIR BIT_DEPTH
//
// DIR holds meta.txt (width height pictures requests slices), y.raw / cb.raw / cr.raw (pictures x
// plane samples: uint8 at 8 bits, uint16 at 10), params.raw (fme_skip_params per slice),
// slice.raw (int32 per request: its slice), reqs.raw (fme_skip_req), res.raw (fme_skip_res).
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

template <typename T>
void set_pictures(fme_hm::MotionCompensator& mc, const std::string& dir, int width, int height, int npic) {
  const size_t plane = (size_t)width * height, cplane = (size_t)(width / 2) * (height / 2);
  const auto y = read_raw<T>(dir + "/y.raw", plane * npic);
  const auto cb = read_raw<T>(dir + "/cb.raw", cplane * npic);
  const auto cr = read_raw<T>(dir + "/cr.raw", cplane * npic);
  for (int k = 0; k < npic; k++) {
    if constexpr (sizeof(T) == 2)
      mc.setPictureYuv16(k, y.data() + plane * k, width, cb.data() + cplane * k, cr.data() + cplane * k, width / 2, width,
                         height);
    else
      mc.setPictureYuv8(k, y.data() + plane * k, width, cb.data() + cplane * k, cr.data() + cplane * k, width / 2, width,
                        height);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s DIR BIT_DEPTH\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int bit_depth = std::atoi(argv[2]);
  int width = 0, height = 0, npic = 0, nreq = 0, nslice = 0;
  {
    FILE* f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d %d %d", &width, &height, &npic, &nreq, &nslice) != 5) {
      std::fprintf(stderr, "bad meta.txt\n");
      return 2;
    }
    std::fclose(f);
  }
  try {
    fme_hm::SearchConfig cfg;
    cfg.nnMode = 0;
    cfg.bitDepth = bit_depth;
    fme_hm::FracSearch search(cfg);
    fme_hm::MotionCompensator mc(search);
    if (bit_depth > 8) set_pictures<uint16_t>(mc, dir, width, height, npic);
    else set_pictures<uint8_t>(mc, dir, width, height, npic);
    const auto params = read_raw<fme_skip_params>(dir + "/params.raw", (size_t)nslice);
    const auto slice = read_raw<int32_t>(dir + "/slice.raw", (size_t)nreq);
    const auto reqs = read_raw<fme_skip_req>(dir + "/reqs.raw", (size_t)nreq);
    const auto want = read_raw<fme_skip_res>(dir + "/res.raw", (size_t)nreq);

    fme_hm::SkipEstimator est(search);
    int bad = 0, seen = 0;
    for (int s = 0; s < nslice; s++) {
      std::vector<int> idx;
      for (int i = 0; i < nreq; i++)
        if (slice[i] == s) {
          if (est.add(reqs[i]) != (int)idx.size()) {
            std::fprintf(stderr, "add: index %d\n", i);
            return 1;
          }
          idx.push_back(i);
        }
      const std::vector<fme_skip_res> got = est.run(params[s]);
      if (got.size() != idx.size() || est.pending() != 0) {
        std::fprintf(stderr, "run: %zu results of %zu, %d pending\n", got.size(), idx.size(), est.pending());
        return 1;
      }
      for (size_t k = 0; k < idx.size(); k++) {
        const fme_skip_res& g = got[k];
        const fme_skip_res& w = want[idx[k]];
        if (std::memcmp(&g, &w, sizeof(fme_skip_res)) != 0 && bad++ < 5)
          std::fprintf(stderr, "request %d: best %d/%d best_cost %.17g/%.17g dist0 %u/%u\n", idx[k], g.best, w.best,
                       g.best_cost, w.best_cost, g.cand_dist[0], w.cand_dist[0]);
      }
      seen += (int)idx.size();
    }
    if (bad || seen != nreq) {
      std::fprintf(stderr, "%d of %d requests differ (%d replayed)\n", bad, nreq, seen);
      return 1;
    }
    // an empty queue returns no results; an invalid request throws fme_hm::Error with the library's
    // code and leaves the queue empty
    if (!est.run(params[0]).empty()) return 1;
    fme_skip_req inv = reqs[0];
    inv.n_cand = 6;
    est.add(inv);
    bool threw = false;
    try {
      est.run(params[0]);
    } catch (const fme_hm::Error& e) {
      threw = e.code() == FME_E_INVALID;
    }
    if (!threw || est.pending() != 0) {
      std::fprintf(stderr, "an invalid request did not throw FME_E_INVALID\n");
      return 1;
    }
    std::printf("skip adapter ok: %d requests in %d slices at bit depth %d\n", nreq, nslice, bit_depth);
  } catch (const fme_hm::Error& e) {
    std::fprintf(stderr, "fme_hm::Error %d: %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
