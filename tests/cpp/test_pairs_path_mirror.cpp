// The pairs_path option of galah::FinchPreclusterer (include/galah_finch.hpp)
// through libgalahgpu.so on the GPU: distances() and galah::cluster under
// every path equal the results without the option, an unknown path throws,
// and galah::pairs_matrix of a few rows equals the pairs it must find.
// argv[1] = the golden data directory, argv[2..] = the genome names
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "galah_finch.hpp"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s DATA_DIR NAME...\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  std::vector<std::string> paths;
  for (int a = 2; a < argc; ++a) paths.push_back(dir + "/" + argv[a] + ".gz");
  galah::info_sink() = nullptr;

  galah::FinchPreclusterer plain(0.9f);
  CHECK(plain.pairs_path == -1);
  const auto d_exp = plain.distances(paths);
  galah::FinchClusterer clu(0.95f);
  const auto c_exp = galah::cluster(paths, plain, clu);
  CHECK(d_exp.size() > 0 && c_exp.size() > 1 && c_exp.size() < paths.size());
  for (int path : {GG_PAIRS_PATH_DEFAULT, GG_PAIRS_PATH_MATRIX, GG_PAIRS_PATH_AUTO}) {
    galah::FinchPreclusterer pre(0.9f, 1000, 21, path);
    CHECK(pre.distances(paths) == d_exp);
    CHECK(galah::cluster(paths, pre, clu) == c_exp);
  }
  // a debug sink keeps the streaming call: every compared pair is logged, the result is the same
  size_t logged = 0;
  galah::debug_sink() = [&](const std::string&) { ++logged; };
  CHECK(galah::FinchPreclusterer(0.9f, 1000, 21, GG_PAIRS_PATH_MATRIX).distances(paths) == d_exp);
  galah::debug_sink() = nullptr;
  CHECK(logged == paths.size() * (paths.size() - 1) / 2);

  gg_status cs = GG_OK;
  gg_ctx* probe = gg_create_multi(21, 1000, 0, nullptr, 0, &cs);
  CHECK(probe);
  const bool one_device = gg_device_count(probe) == 1;  // (several devices: the option is ignored)
  gg_destroy(probe);
  if (one_device) {
    galah::FinchPreclusterer bad(0.9f, 1000, 21, 3);
    bool threw = false;
    try {
      bad.distances(paths);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
      galah::cluster(paths, bad, clu);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
  }

  // rows 0 and 2 share 3 of 4 hashes, row 1 shares nothing
  const std::vector<uint64_t> sk = {10, 20, 30, 40, 11, 21, 31, 41, 10, 20, 30, 50};
  const std::vector<uint32_t> lens = {4, 4, 4};
  gg_pairs_matrix_summary sum{};
  const auto all = galah::pairs_matrix(sk, lens, 4, 0.0f, nullptr, 21, &sum);
  CHECK(all.size() == 3 && sum.n_pairs == 3 && sum.n_columns == 3 && sum.path == GG_PAIRS_PATH_MATRIX);
  CHECK(all[1].i == 0 && all[1].j == 2 && all[1].common == 3);
  const std::vector<uint32_t> rows = {2, 1};
  const auto two = galah::pairs_matrix(sk, lens, 4, 0.0f, &rows);
  CHECK(two.size() == 1 && two[0].i == 1 && two[0].j == 2 && two[0].common == 0);
  std::printf("ok\n");
  return 0;
}
