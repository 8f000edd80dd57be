// GPU test driver of fme_hm::CostSurface (include/fme_hm.hpp): a surface fixture exported as raw
// arrays by tests/test_gpu_surface.py, replayed through the adapter and compared word by word.
//
//   test_surface_adapter DIR BIT_DEPTH USE_HADAMARD
//
// DIR holds meta.txt (width height pictures jobs keys lambdas), pictures.raw (pictures x plane
// samples: uint8 at 8 bits, uint16 at 10), keys.raw (int16), lambdas.raw (double), jobs.raw
// (fme_job), probes.raw (2 bytes per job), surf.raw (fme_surface: the expected words).
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
    cfg.nnMode = 0;
    cfg.bitDepth = bit_depth;
    cfg.useHadamardME = std::atoi(argv[3]) != 0;
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
    if (fme_set_keys(search.ctx(), keys.data(), keys.size(), nullptr) != FME_OK) {
      std::fprintf(stderr, "fme_set_keys: %s\n", fme_last_error());
      return 1;
    }
    const auto jobs = read_raw<fme_job>(dir + "/jobs.raw", (size_t)njob);
    const auto probes = read_raw<uint8_t>(dir + "/probes.raw", 2 * (size_t)njob);
    const auto want = read_raw<fme_surface>(dir + "/surf.raw", (size_t)njob);

    fme_hm::CostSurface cs(search);
    for (int i = 0; i < njob; i++)
      if (cs.add(jobs[i], probes[2 * i], probes[2 * i + 1]) != i) {
        std::fprintf(stderr, "add: index %d\n", i);
        return 1;
      }
    std::vector<fme_surface> surf;
    const std::vector<fme_surface_pick> picks = cs.run(&surf);
    if ((int)picks.size() != njob || (int)surf.size() != njob || cs.pending() != 0) {
      std::fprintf(stderr, "run: %zu picks, %zu surfaces of %d, %d pending\n", picks.size(), surf.size(), njob, cs.pending());
      return 1;
    }
    int bad = 0;
    for (int i = 0; i < njob; i++) {
      const fme_surface_pick& p = picks[i];
      bool ok = std::memcmp(&surf[i], &want[i], sizeof(fme_surface)) == 0 && p.status == 0;
      int first = 0;
      for (int k = 1; k < FME_SURF_POINTS; k++)
        if (want[i].cost[k] < want[i].cost[first]) first = k;
      ok = ok && p.min_idx == first && p.min_cost == want[i].cost[first];
      for (int k = 0; k < 2; k++) {
        const uint8_t pr = probes[2 * i + k];
        ok = ok && p.probe[k] == pr && p.probe_cost[k] == (pr == FME_SURF_NO_PROBE ? 0xFFFFFFFFu : want[i].cost[pr]);
      }
      if (!ok && bad++ < 5)
        std::fprintf(stderr, "job %d: dist0 %u/%u cost0 %u/%u min %u@%d/%u@%d\n", i, surf[i].dist[0], want[i].dist[0],
                     surf[i].cost[0], want[i].cost[0], p.min_cost, p.min_idx, want[i].cost[first], first);
    }
    if (bad) {
      std::fprintf(stderr, "%d of %d jobs differ\n", bad, njob);
      return 1;
    }
    // picks alone equal the picks beside surfaces
    for (int i = 0; i < njob; i++) cs.add(jobs[i], probes[2 * i], probes[2 * i + 1]);
    const std::vector<fme_surface_pick> alone = cs.run();
    if (alone.size() != picks.size() || std::memcmp(alone.data(), picks.data(), picks.size() * sizeof(fme_surface_pick)) != 0) {
      std::fprintf(stderr, "picks without surfaces differ\n");
      return 1;
    }
    // an empty queue returns no picks; an invalid job throws fme_hm::Error with the library's code
    // and leaves the queue empty
    if (!cs.run().empty()) return 1;
    fme_job inv = jobs[0];
    inv.w = 6;
    cs.add(inv);
    bool threw = false;
    try {
      cs.run();
    } catch (const fme_hm::Error& e) {
      threw = e.code() == FME_E_INVALID;
    }
    if (!threw || cs.pending() != 0) {
      std::fprintf(stderr, "an invalid job did not throw FME_E_INVALID\n");
      return 1;
    }
    std::printf("surface adapter ok: %d jobs at bit depth %d\n", njob, bit_depth);
  } catch (const fme_hm::Error& e) {
    std::fprintf(stderr, "fme_hm::Error %d: %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
