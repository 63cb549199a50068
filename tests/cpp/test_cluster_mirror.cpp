// galah::cluster (include/galah_finch.hpp) for finch + finch, through
// libgalahgpu.so on the GPU.  Built and run by
// tests/test_cluster_gpu.py.
// argv[1] = the golden data directory, argv[2] = the expected rep_of of the
// golden genomes at precluster ANI 0.9 / cluster ANI 0.95 (comma-separated),
// argv[3..] = the genome names in golden order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "galah_finch.hpp"

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// a clusterer galah has and this library does not run
struct Skani : galah::FinchClusterer {
  using galah::FinchClusterer::FinchClusterer;
  const char* method_name() const override { return "skani"; }
};

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s DATA_DIR REP_OF NAME...\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  std::vector<uint32_t> rep_of;
  for (const char* p = argv[2]; *p;) {
    char* end = nullptr;
    rep_of.push_back((uint32_t)std::strtoul(p, &end, 10));
    p = *end == ',' ? end + 1 : end;
  }
  std::vector<std::string> paths;
  for (int a = 3; a < argc; ++a) paths.push_back(dir + "/" + argv[a] + ".gz");
  CHECK(rep_of.size() == paths.size());

  // the expected clusters: by representative ascending, it first, members ascending
  std::vector<std::vector<size_t>> expected;
  for (size_t r = 0; r < rep_of.size(); ++r) {
    if (rep_of[r] != r) continue;
    expected.push_back({r});
    for (size_t g = 0; g < rep_of.size(); ++g)
      if (g != r && rep_of[g] == r) expected.back().push_back(g);
  }

  galah::FinchPreclusterer pre(0.9f, 1000, 21);
  galah::FinchClusterer clu(0.95f);
  CHECK(std::strcmp(clu.method_name(), "finch") == 0 && clu.get_ani_threshold() == 0.95f);
  std::vector<std::string> log;
  galah::info_sink() = [&](const std::string& line) { log.push_back(line); };
  const auto clusters = galah::cluster(paths, pre, clu);
  galah::info_sink() = nullptr;
  CHECK(clusters == expected);
  CHECK(clusters.size() == 5);
  // src/clusterer.rs:24-32
  CHECK(log.size() >= 2 && log[0] == "Preclustering with finch and clustering with finch");
  CHECK(log.size() >= 2 && log[1] == "Preclustering and clustering methods are the same, so reusing ANI values");

  Skani other(0.95f);
  bool threw = false;
  try {
    galah::cluster(paths, pre, other);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);

  // src/finch.rs:96
  const auto a = clu.calculate_ani(dir + "/set1/1mbp.fna.gz", dir + "/set1/500kb.fna.gz");
  CHECK(a && *a == 0.9808188f);

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
