// galah::validate_clusters, read_clustering_file and the two writers
// (include/galah_finch.hpp) through libgalahgpu.so on the GPU: the round trip
// from files.  Built and run by tests/test_validate_gpu.py.
// argv[1] = the golden data directory, argv[2] = a scratch directory,
// argv[3..] = the genome names in golden order.
// Prints "ok", then the error lines of the validation at 0.98, each after "E ".
#include <cstdio>
#include <fstream>
#include <sstream>
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

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s DATA_DIR SCRATCH_DIR NAME...\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1], scratch = argv[2];
  std::vector<std::string> paths;
  for (int a = 3; a < argc; ++a) paths.push_back(dir + "/" + argv[a] + ".gz");

  galah::info_sink() = nullptr;
  galah::FinchPreclusterer pre(0.9f, 1000, 21);
  galah::FinchClusterer clu(0.95f);
  const auto clusters = galah::cluster(paths, pre, clu);
  CHECK(clusters.size() == 5);

  // writers: the bytes, and read(write(x)) == x
  std::ostringstream text;
  galah::write_cluster_definition(text, clusters, paths);
  std::string expected;
  std::vector<std::vector<std::string>> named;
  for (const auto& c : clusters) {
    named.emplace_back();
    for (size_t g : c) {
      expected += paths[c[0]] + "\t" + paths[g] + "\n";
      named.back().push_back(paths[g]);
    }
  }
  CHECK(text.str() == expected);
  std::ostringstream reps;
  galah::write_representative_list(reps, clusters, paths);
  CHECK(reps.str() == paths[clusters[0][0]] + "\n" + paths[clusters[1][0]] + "\n" + paths[clusters[2][0]] + "\n" +
                          paths[clusters[3][0]] + "\n" + paths[clusters[4][0]] + "\n");
  const std::string file = scratch + "/clusters.tsv";
  {
    std::ofstream f(file, std::ios::binary);
    galah::write_cluster_definition(f, clusters, paths);
  }
  CHECK(galah::read_clustering_file(file) == named);

  // the reader's rules
  {
    std::ofstream f(scratch + "/odd.tsv", std::ios::binary);
    f << "x\ty\n\na\ta\nq\tb\r\nc\tc\n";
  }
  CHECK((galah::read_clustering_file(scratch + "/odd.tsv") ==
         std::vector<std::vector<std::string>>{{"a", "b"}, {"c"}}));
  {
    std::ofstream f(scratch + "/three.tsv", std::ios::binary);
    f << "a\ta\na\tb\tc\n";
  }
  bool threw = false;
  try {
    galah::read_clustering_file(scratch + "/three.tsv");
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  // validation at the clustering's own threshold, then at a tighter one
  std::vector<std::string> info, errors;
  galah::info_sink() = [&](const std::string& line) { info.push_back(line); };
  galah::error_sink() = [&](const std::string& line) { errors.push_back(line); };
  const galah::ClusterValidation same = galah::validate_clusters(file, 0.95f);
  CHECK(same.ok() && same.member_pairs == 22 && same.rep_pairs == 10);
  CHECK(errors.empty());
  CHECK(!info.empty() && info[0] == "Read in 5 clusters");
  const galah::ClusterValidation tight = galah::validate_clusters(file, 0.98f);
  CHECK(!tight.ok() && tight.member_pairs == 22 && tight.rep_pairs == 10);
  CHECK(!tight.member_bad.empty() && tight.rep_bad.empty());
  CHECK(errors.size() == tight.member_bad.size());
  for (const auto& v : tight.member_bad) CHECK(v.ani < 0.98f);

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  for (const auto& e : errors) std::printf("E %s\n", e.c_str());
  return 0;
}
