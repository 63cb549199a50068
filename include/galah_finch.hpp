// galah_finch.hpp -- C++ mirror of galah's finch precluster interface over
// the C ABI of libgalahgpu.so (galahgpu.h).  Header-only.
//
//   reference (AroneyS/galah @ 2024-12-18)               here
//   src/lib.rs:23-27   trait PreclusterDistanceFinder     galah::PreclusterDistanceFinder
//   src/finch.rs:4-24  struct FinchPreclusterer           galah::FinchPreclusterer
//   src/finch.rs:26-75 finch::distances(...)              galah::finch_distances(...)
//   src/lib.rs:29-37   trait ClusterDistanceFinder        galah::ClusterDistanceFinder, FinchClusterer
//   src/clusterer.rs:14-125 cluster(...)                  galah::cluster (finch + finch)
//   src/sorted_pair_genome_distance_cache.rs:4-59         galah::SortedPairGenomeDistanceCache
//   src/cluster_argument_parsing.rs:1160-1182             galah::parse_percentage
//   src/genome_stats.rs:4-51                              galah::GenomeAssemblyStats, calculate_genome_stats
//   src/cluster_validation.rs:7-78                        galah::validate_clusters
//   src/cluster_validation.rs:80-113                      galah::read_clustering_file
//   src/cluster_argument_parsing.rs:437-449, :478-484     galah::write_cluster_definition, write_representative_list
//
// Errors: the reference panics ("Failed to sketch genomes with finch",
// src/finch.rs:50); here the same message is thrown as std::runtime_error.
#pragma once

#include <algorithm>
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <functional>
#include <map>
#include <ostream>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "galahgpu.h"

namespace galah {

// src/sorted_pair_genome_distance_cache.rs: BTreeMap<(usize,usize), Option<f32>>
// with keys normalised to (min, max).
class SortedPairGenomeDistanceCache {
 public:
  using Key = std::pair<size_t, size_t>;

  void insert(Key ids, std::optional<float> distance) { internal_[norm(ids)] = distance; }
  // Option<&Option<f32>>: nullptr when absent
  const std::optional<float>* get(Key ids) const {
    auto it = internal_.find(norm(ids));
    return it == internal_.end() ? nullptr : &it->second;
  }
  bool contains_key(Key ids) const { return internal_.count(norm(ids)) != 0; }
  // :47-58
  SortedPairGenomeDistanceCache transform_ids(const std::vector<size_t>& input_ids) const {
    SortedPairGenomeDistanceCache out;
    for (size_t i = 0; i < input_ids.size(); ++i)
      for (size_t j = i + 1; j < input_ids.size(); ++j)
        if (const auto* v = get({input_ids[i], input_ids[j]})) out.insert({i, j}, *v);
    return out;
  }
  size_t size() const { return internal_.size(); }
  const std::map<Key, std::optional<float>>& internal() const { return internal_; }
  bool operator==(const SortedPairGenomeDistanceCache& o) const { return internal_ == o.internal_; }

 private:
  static Key norm(Key k) { return k.first < k.second ? k : Key{k.second, k.first}; }
  std::map<Key, std::optional<float>> internal_;
};

// src/lib.rs:23-27
class PreclusterDistanceFinder {
 public:
  virtual ~PreclusterDistanceFinder() = default;
  virtual SortedPairGenomeDistanceCache distances(const std::vector<std::string>& genome_fasta_paths) = 0;
  virtual const char* method_name() const = 0;
};

// CAP:1160-1182 (the --precluster-ani value)
inline float parse_percentage(float value) {
  float out = 0.f;
  if (gg_parse_percentage(value, &out) != GG_OK) throw std::invalid_argument(gg_thread_last_error());
  return out;
}

// rayon's global pool, which galah builds with --threads threads
// (CAP:408-412, default 1); finch_distances reads its size the way the Rust
// body in INTEGRATION.md calls rayon::current_num_threads().  0 = unset: the
// machine's CPUs, rayon's own default.
inline int& rayon_pool_slot() {
  static int n = 0;
  return n;
}
inline void set_num_threads(int n) { rayon_pool_slot() = n > 0 ? n : 0; }
inline int current_num_threads() {
  const int n = rayon_pool_slot();
  return n > 0 ? n : (int)std::max(1u, std::thread::hardware_concurrency());
}

// galah's info! log (env_logger, shown at the default level): the two lines
// of src/finch.rs:46,48 plus one line from the library (gg_info_line: device
// count, phase times, fallbacks).  The sink is replaceable (tests capture it);
// the default writes to stderr as env_logger would.
inline std::function<void(const std::string&)>& info_sink() {
  static std::function<void(const std::string&)> sink = [](const std::string& line) {
    std::fprintf(stderr, "[INFO] %s\n", line.c_str());
  };
  return sink;
}
inline void info(const std::string& line) {
  if (info_sink()) info_sink()(line);
}

// galah's debug! log: unset (the default level, info) logs nothing; set, it
// receives src/finch.rs:65-68's line for every compared pair.
inline std::function<void(const std::string&)>& debug_sink() {
  static std::function<void(const std::string&)> sink;
  return sink;
}

// Rust's `{}` of an f64: the shortest digits that read back the same value,
// fixed notation (1.0 -> "1", 1e-7 -> "0.0000001")
inline std::string rust_f64(double x) {
  char buf[400];
  const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

namespace detail {
// sketch + all pairs + threshold on an existing context; takes ownership of ctx
// pairs_path >= 0 (GG_PAIRS_PATH_*): the resident call under that path, on a
// one-device context and below debug level; the result is the same
inline SortedPairGenomeDistanceCache distances_on(gg_ctx* ctx, const std::vector<std::string>& paths, float min_ani,
                                                  int kmer_length, int pairs_path = -1) {
  if (!ctx)
    throw std::runtime_error(std::string("Failed to sketch genomes with finch: ") + gg_thread_last_error());
  gg_set_host_threads(ctx, current_num_threads());
  std::vector<const char*> c_paths;
  for (const auto& p : paths) c_paths.push_back(p.c_str());
  gg_pair* pairs = nullptr;
  float* ani = nullptr;
  uint64_t n = 0;
  info("Sketching MinHash representations of each genome with finch ..");  // src/finch.rs:46
  // at debug level every compared pair is logged (src/finch.rs:65-68): the
  // library streams all N (N - 1) / 2 of them in row blocks, in the
  // reference's loop order, while the returned pairs are those >= min_ani
  struct Each {
    const std::vector<std::string>* paths;
    int k;
    static int sink(void* user, const gg_pair* p, uint64_t n) {
      const Each* e = (const Each*)user;
      for (uint64_t x = 0; x < n; ++x)
        debug_sink()("Comparing " + (*e->paths)[p[x].i] + " and " + (*e->paths)[p[x].j] + ", distance " +
                     rust_f64(gg_ani_f64(p[x].common, p[x].total, e->k)));
      return 0;
    }
  } each{&paths, kmer_length};
  const bool resident = !debug_sink() && pairs_path >= 0 && gg_device_count(ctx) == 1;
  gg_status st = resident ? gg_set_pairs_path(ctx, pairs_path) : GG_OK;  // (an unknown path is an error)
  if (st == GG_OK) {
    if (debug_sink())
      st = gg_precluster_files_each(ctx, c_paths.data(), (uint32_t)c_paths.size(), min_ani, nullptr, &Each::sink, &each,
                                    &pairs, &ani, &n, nullptr);
    else if (resident)
      st = gg_precluster_files_resident(ctx, c_paths.data(), (uint32_t)c_paths.size(), min_ani, nullptr, &pairs, &ani,
                                        &n, nullptr);
    else
      st = gg_precluster_files(ctx, c_paths.data(), (uint32_t)c_paths.size(), min_ani, &pairs, &ani, &n);
  }
  if (st != GG_OK) {
    std::string msg = gg_last_error(ctx);
    gg_destroy(ctx);
    throw std::runtime_error("Failed to sketch genomes with finch: " + msg);  // src/finch.rs:50
  }
  info("Finished sketching genomes");  // src/finch.rs:48 (sketches and pairs come from one call here)
  char line[1024];
  if (gg_info_line(ctx, line, sizeof line) == GG_OK) info(line);
  SortedPairGenomeDistanceCache cache;
  for (uint64_t i = 0; i < n; ++i) cache.insert({pairs[i].i, pairs[i].j}, ani[i]);  // src/finch.rs:70
  gg_free(pairs);
  gg_free(ani);
  gg_destroy(ctx);
  return cache;
}
}  // namespace detail

// src/finch.rs:26-75 on the GPU, same arguments: sketch (K1), all pairs (K2),
// keep ani >= min_ani.  Every visible GPU (or GALAHGPU_DEVICES), as galah's
// one distances() call would use them; file ingest on current_num_threads().
inline SortedPairGenomeDistanceCache finch_distances(const std::vector<std::string>& paths, float min_ani,
                                                     size_t num_kmers, uint8_t kmer_length) {
  gg_status st = GG_OK;
  return detail::distances_on(gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, nullptr, 0, &st), paths, min_ani,
                              kmer_length);
}

// The same on one HIP device (ordinal; -1 = the current device).
inline SortedPairGenomeDistanceCache finch_distances(const std::vector<std::string>& paths, float min_ani,
                                                     size_t num_kmers, uint8_t kmer_length, int device) {
  gg_status st = GG_OK;
  return detail::distances_on(gg_create(kmer_length, (uint32_t)num_kmers, 0, device, &st), paths, min_ani, kmer_length);
}

// The same on a list of HIP ordinals (repeats allowed: several members on one GPU).
inline SortedPairGenomeDistanceCache finch_distances_on(const std::vector<int>& devices,
                                                        const std::vector<std::string>& paths, float min_ani,
                                                        size_t num_kmers, uint8_t kmer_length) {
  gg_status st = GG_OK;
  return detail::distances_on(
      gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, devices.data(), (uint32_t)devices.size(), &st), paths,
      min_ani, kmer_length);
}

// src/finch.rs:4-24.  pairs_path: -1 (the default K2 through the calls used so
// far) or GG_PAIRS_PATH_DEFAULT / _MATRIX / _AUTO: distances() and
// galah::cluster then take the resident calls under that pairs path
// (gg_set_pairs_path; MATRIX suits thousands of strains of one species).  The
// results do not depend on it; it is ignored on a multi-device context and,
// in distances(), when a debug sink is set (every compared pair is logged).
class FinchPreclusterer : public PreclusterDistanceFinder {
 public:
  FinchPreclusterer(float min_ani, size_t num_kmers = 1000, uint8_t kmer_length = 21, int pairs_path = -1)
      : min_ani(min_ani), num_kmers(num_kmers), kmer_length(kmer_length), pairs_path(pairs_path) {}
  SortedPairGenomeDistanceCache distances(const std::vector<std::string>& paths) override {
    if (pairs_path < 0) return finch_distances(paths, min_ani, num_kmers, kmer_length);
    gg_status st = GG_OK;
    return detail::distances_on(gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, nullptr, 0, &st), paths, min_ani,
                                kmer_length, pairs_path);
  }
  const char* method_name() const override { return "finch"; }

  float min_ani;  // fraction, not percentage
  size_t num_kmers;
  uint8_t kmer_length;
  int pairs_path;
};

// src/lib.rs:29-37
class ClusterDistanceFinder {
 public:
  virtual ~ClusterDistanceFinder() = default;
  virtual void initialise() = 0;
  virtual const char* method_name() const = 0;
  virtual float get_ani_threshold() const = 0;
  virtual std::optional<float> calculate_ani(const std::string& fasta1, const std::string& fasta2) = 0;
};

// A finch clusterer: its value for a pair is the one FinchPreclusterer
// stores (the original design of src/clusterer.rs, find_minhash_representatives
// / find_minhash_memberships; galah's CLUSTER_METHODS has no finch).
class FinchClusterer : public ClusterDistanceFinder {
 public:
  FinchClusterer(float ani, size_t num_kmers = 1000, uint8_t kmer_length = 21)
      : ani(ani), num_kmers(num_kmers), kmer_length(kmer_length) {}
  void initialise() override {}
  const char* method_name() const override { return "finch"; }
  float get_ani_threshold() const override { return ani; }
  // the two files through finch_distances at min_ani 0 (info lines muted)
  std::optional<float> calculate_ani(const std::string& fasta1, const std::string& fasta2) override {
    auto saved = info_sink();
    info_sink() = nullptr;
    SortedPairGenomeDistanceCache d;
    try {
      d = finch_distances({fasta1, fasta2}, 0.0f, num_kmers, kmer_length);
    } catch (...) {
      info_sink() = saved;
      throw;
    }
    info_sink() = saved;
    const auto* v = d.get({0, 1});
    return v ? *v : std::nullopt;
  }

  float ani;  // fraction, not percentage
  size_t num_kmers;
  uint8_t kmer_length;
};

// src/clusterer.rs:14-125 -> the clusters as lists of genome indices, each
// with its representative first, by representative ascending (the reference
// assembles its list in rayon completion order, :114-121).  Built for the
// case the reference marks skip_clusterer (:29-33): a FinchPreclusterer with
// a clusterer whose method_name() is also "finch", the result then being a
// function of the pair cache, computed on the GPU (gg_cluster_files).  Any
// other combination throws std::invalid_argument: the external-clusterer flow
// is not part of this library.
inline std::vector<std::vector<size_t>> cluster(const std::vector<std::string>& genomes,
                                                PreclusterDistanceFinder& preclusterer,
                                                ClusterDistanceFinder& clusterer) {
  clusterer.initialise();
  const std::string pre_name = preclusterer.method_name(), clu_name = clusterer.method_name();
  info("Preclustering with " + pre_name + " and clustering with " + clu_name);  // :24-27
  const auto* finch = dynamic_cast<const FinchPreclusterer*>(&preclusterer);
  if (!finch || pre_name != "finch" || clu_name != "finch")
    throw std::invalid_argument("galah::cluster: only finch + finch (the clusterer reusing the preclusterer's ANI "
                                "values) runs here, not " + pre_name + " + " + clu_name);
  info("Preclustering and clustering methods are the same, so reusing ANI values");  // :31
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(finch->kmer_length, (uint32_t)finch->num_kmers, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(std::string("Failed to sketch genomes with finch: ") + gg_thread_last_error());
  gg_set_host_threads(ctx, current_num_threads());
  std::vector<const char*> c_paths;
  for (const auto& p : genomes) c_paths.push_back(p.c_str());
  const uint32_t n = (uint32_t)genomes.size();
  std::vector<uint32_t> rep_of(n), members(n), offsets((size_t)n + 1);
  info("Sketching MinHash representations of each genome with finch ..");  // src/finch.rs:46
  if (finch->pairs_path >= 0 && gg_device_count(ctx) == 1) {  // the resident call under the preclusterer's path
    st = gg_set_pairs_path(ctx, finch->pairs_path);
    if (st == GG_OK)
      st = gg_cluster_files_resident(ctx, c_paths.data(), n, finch->min_ani, clusterer.get_ani_threshold(), nullptr,
                                     rep_of.data(), nullptr);
  } else {
    st = gg_cluster_files(ctx, c_paths.data(), n, finch->min_ani, clusterer.get_ani_threshold(), nullptr,
                          rep_of.data(), nullptr, nullptr, nullptr);
  }
  if (st != GG_OK) {
    const std::string msg = gg_last_error(ctx);
    gg_destroy(ctx);
    throw std::runtime_error("Failed to sketch genomes with finch: " + msg);  // src/finch.rs:50
  }
  info("Finished sketching genomes");  // src/finch.rs:48
  char line[1024];
  if (gg_info_line(ctx, line, sizeof line) == GG_OK) info(line);
  gg_destroy(ctx);
  info("Finding representative genomes and assigning all genomes to these ..");  // :65
  uint32_t nc = 0;
  if (gg_clusters_from_reps(n, rep_of.data(), members.data(), offsets.data(), &nc) != GG_OK)
    throw std::runtime_error(gg_thread_last_error());
  std::vector<std::vector<size_t>> out(nc);
  for (uint32_t c = 0; c < nc; ++c) out[c].assign(members.begin() + offsets[c], members.begin() + offsets[c + 1]);
  return out;
}

// ---- cluster definition files and their validation -------------------------

// src/cluster_argument_parsing.rs:437-449 (--output-cluster-definition): for
// every cluster, for every genome of it (the representative first, as
// itself), "<representative>\t<genome>\n".
inline void write_cluster_definition(std::ostream& f, const std::vector<std::vector<size_t>>& clusters,
                                     const std::vector<std::string>& genomes) {
  for (const auto& cluster : clusters)
    for (size_t g : cluster) f << genomes[cluster[0]] << '\t' << genomes[g] << '\n';
}

// src/cluster_argument_parsing.rs:478-484 (--output-representative-list)
inline void write_representative_list(std::ostream& f, const std::vector<std::vector<size_t>>& clusters,
                                      const std::vector<std::string>& genomes) {
  for (const auto& cluster : clusters) f << genomes[cluster[0]] << '\n';
}

// src/cluster_validation.rs:80-113: tab-separated, exactly two fields per
// line (std::runtime_error otherwise, where the reference exits); a line
// whose two fields are equal opens a cluster; lines before the first such
// line are dropped; a member line's first field is not compared with the open
// representative; empty lines are skipped.  Unlike the reference's csv
// reader, CSV quoting is not interpreted.
inline std::vector<std::vector<std::string>> read_clustering_file(const std::string& clustering_file) {
  std::ifstream in(clustering_file, std::ios::binary);
  if (!in) throw std::runtime_error("Failed to open clustering file: " + clustering_file);  // :84
  std::vector<std::vector<std::string>> all_clusters;
  std::vector<std::string> current_cluster;
  bool have_rep = false;
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos || line.find('\t', tab + 1) != std::string::npos)
      throw std::runtime_error("Unexpectedly didn't find exactly 2 fields in clustering file: " + line);  // :93-96
    const std::string first = line.substr(0, tab), second = line.substr(tab + 1);
    if (first == second) {
      if (have_rep) all_clusters.push_back(current_cluster);
      current_cluster.clear();
      have_rep = true;
    }
    current_cluster.push_back(second);
  }
  if (have_rep) all_clusters.push_back(current_cluster);
  return all_clusters;
}

// galah's error! log: validate_clusters' "not ok" lines.  Replaceable; the
// default writes to stderr as env_logger would.
inline std::function<void(const std::string&)>& error_sink() {
  static std::function<void(const std::string&)> sink = [](const std::string& line) {
    std::fprintf(stderr, "[ERROR] %s\n", line.c_str());
  };
  return sink;
}

// Rust's `{}` of an f32 (the shortest digits that read back the same value)
inline std::string rust_f32(float x) {
  char buf[80];
  const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);
  return std::string(buf, r.ptr);
}

// One violation: two paths of the file and the pair's f32 ANI (a fraction).
struct ClusterViolation {
  std::string first, second;
  float ani;
};
struct ClusterValidation {
  uint64_t member_pairs = 0, rep_pairs = 0;
  std::vector<ClusterViolation> member_bad;  // (representative, member), below the threshold
  std::vector<ClusterViolation> rep_bad;     // two representatives at or above it
  bool ok() const { return member_bad.empty() && rep_bad.empty(); }
};

// src/cluster_validation.rs:7-78 (galah cluster-validate) with finch's ANI in
// FastANI's place, on the GPU (gg_validate_files): the file is read, every
// distinct path sketched once, every member checked against its
// representative (>= ani_threshold, a fraction) and every pair of
// representatives (< ani_threshold), f32 against f32.  Logs the reference's
// lines with "finch ANI" for "FastANI" and the values as it prints them
// (percent: ani * 100 in f32): "Read in {} clusters" to info, the "not ok"
// lines to error_sink (the "ok" lines of the debug level are not made here).
inline ClusterValidation validate_clusters(const std::string& clustering_file, float ani_threshold,
                                           size_t num_kmers = 1000, uint8_t kmer_length = 21,
                                           const char* sketch_cache_dir = nullptr) {
  const auto clusters = read_clustering_file(clustering_file);
  info("Read in " + std::to_string(clusters.size()) + " clusters");  // :17
  std::map<std::string, uint32_t> index;
  std::vector<const char*> c_paths;
  std::vector<uint32_t> members, offsets{0};
  for (const auto& cluster : clusters) {
    for (const auto& path : cluster) {
      auto it = index.find(path);
      if (it == index.end()) {
        it = index.emplace(path, (uint32_t)c_paths.size()).first;
        c_paths.push_back(it->first.c_str());  // (map nodes do not move)
      }
      members.push_back(it->second);
    }
    offsets.push_back((uint32_t)members.size());
  }
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(std::string("Failed to sketch genomes with finch: ") + gg_thread_last_error());
  gg_set_host_threads(ctx, current_num_threads());
  gg_validation sum{};
  gg_pair* bad = nullptr;
  float* bad_ani = nullptr;
  uint64_t n_bad = 0;
  st = gg_validate_files(ctx, c_paths.data(), (uint32_t)c_paths.size(), members.data(), offsets.data(),
                         (uint32_t)clusters.size(), ani_threshold, sketch_cache_dir, &sum, &bad, &bad_ani, &n_bad);
  if (st != GG_OK) {
    const std::string msg = gg_last_error(ctx);
    gg_destroy(ctx);
    throw std::runtime_error("Failed to sketch genomes with finch: " + msg);  // src/finch.rs:50
  }
  gg_destroy(ctx);
  ClusterValidation out;
  out.member_pairs = sum.member_pairs;
  out.rep_pairs = sum.rep_pairs;
  for (uint64_t p = 0; p < n_bad; ++p) {
    const ClusterViolation v{c_paths[bad[p].i], c_paths[bad[p].j], bad_ani[p]};
    const bool member = p < sum.member_bad;
    (member ? out.member_bad : out.rep_bad).push_back(v);
    if (error_sink())  // :31-34, :62-65
      error_sink()(std::string("finch ANI between ") + (member ? "" : "reps ") + v.first + " and " + v.second +
                   " is not ok: " + rust_f32(v.ani * 100.0f));
  }
  gg_free(bad);
  gg_free(bad_ani);
  return out;
}

// The finch ANI between every two of the genomes, as the value galah stores
// for a pair (gg_ani_matrix_files): every file sketched once, then one dense
// matrix call on the GPU.  Row-major [N x N], symmetric, 1 on the diagonal of
// a genome with a non-empty sketch.
inline std::vector<float> ani_matrix(const std::vector<std::string>& paths, size_t num_kmers = 1000,
                                     uint8_t kmer_length = 21, const char* sketch_cache_dir = nullptr) {
  std::vector<float> out(paths.size() * paths.size());
  if (paths.empty()) return out;
  std::vector<const char*> c_paths;
  for (const auto& p : paths) c_paths.push_back(p.c_str());
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(std::string("Failed to sketch genomes with finch: ") + gg_thread_last_error());
  gg_set_host_threads(ctx, current_num_threads());
  st = gg_ani_matrix_files(ctx, c_paths.data(), (uint32_t)c_paths.size(), sketch_cache_dir, nullptr, nullptr,
                           out.data(), nullptr);
  const std::string msg = st != GG_OK ? gg_last_error(ctx) : "";
  gg_destroy(ctx);
  if (st != GG_OK) throw std::runtime_error("Failed to sketch genomes with finch: " + msg);  // src/finch.rs:50
  return out;
}

// The pairs of a sketch matrix at or above min_ani (a fraction), sorted by
// (i, j), by the matrix product with the thresholded epilogue
// (gg_pairs_matrix): gg_pairs' answer, built for dense sets.  sketches is
// [lens.size() x sketch_size], rows ascending; rows (may be null: every row)
// lists the rows to compare, none twice.
inline std::vector<gg_pair> pairs_matrix(const std::vector<uint64_t>& sketches, const std::vector<uint32_t>& lens,
                                         size_t sketch_size, float min_ani, const std::vector<uint32_t>* rows = nullptr,
                                         uint8_t kmer_length = 21, gg_pairs_matrix_summary* summary = nullptr) {
  if (sketches.size() != lens.size() * sketch_size) throw std::invalid_argument("sketches must be [n x sketch_size]");
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(kmer_length, (uint32_t)sketch_size, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(gg_thread_last_error());
  gg_pair* p = nullptr;
  uint64_t n = 0;
  st = gg_pairs_matrix(ctx, sketches.data(), lens.data(), (uint32_t)lens.size(), rows ? rows->data() : nullptr,
                       (uint32_t)(rows ? rows->size() : lens.size()), min_ani, &p, &n, summary);
  const std::string msg = st != GG_OK ? gg_last_error(ctx) : "";
  gg_destroy(ctx);
  if (st != GG_OK) throw std::runtime_error(msg);
  std::vector<gg_pair> out(p, p + n);
  gg_free(p);
  return out;
}

// The hits of queries that are not to be added (gg_query_rows): every cell
// (row i, query q) at or above min_ani (a fraction) as gg_pair{i, lens.size()
// + q, common, total}, sorted by (i, j), with their f32 ANI in *ani (may be
// null).  sketches is [lens.size() x sketch_size], q_sketches [q_lens.size() x
// sketch_size], rows ascending.
inline std::vector<gg_pair> query_rows(const std::vector<uint64_t>& sketches, const std::vector<uint32_t>& lens,
                                       const std::vector<uint64_t>& q_sketches, const std::vector<uint32_t>& q_lens,
                                       size_t sketch_size, float min_ani, std::vector<float>* ani = nullptr,
                                       uint8_t kmer_length = 21) {
  if (sketches.size() != lens.size() * sketch_size || q_sketches.size() != q_lens.size() * sketch_size)
    throw std::invalid_argument("sketches must be [n x sketch_size]");
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(kmer_length, (uint32_t)sketch_size, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(gg_thread_last_error());
  gg_pair* p = nullptr;
  float* a = nullptr;
  uint64_t n = 0;
  st = gg_query_rows(ctx, sketches.data(), lens.data(), (uint32_t)lens.size(), q_sketches.data(), q_lens.data(),
                     (uint32_t)q_lens.size(), min_ani, &p, &a, &n);
  const std::string msg = st != GG_OK ? gg_last_error(ctx) : "";
  gg_destroy(ctx);
  if (st != GG_OK) throw std::runtime_error(msg);
  std::vector<gg_pair> out(p, p + n);
  if (ani) ani->assign(a, a + n);
  gg_free(p);
  gg_free(a);
  return out;
}

// The finch ANI table of every precluster of the genomes
// (gg_precluster_matrices_files): the files sketched once, the preclusters at
// precluster_ani (a fraction) and each one's dense matrix in one grouped call
// on the GPU.  Largest precluster first; a block is row-major [m x m] over
// `indices` (into paths, ascending).
struct PreclusterAniMatrix {
  std::vector<size_t> indices;
  std::vector<float> ani;
};
inline std::vector<PreclusterAniMatrix> precluster_ani_matrices(const std::vector<std::string>& paths,
                                                                float precluster_ani = 0.9f, size_t num_kmers = 1000,
                                                                uint8_t kmer_length = 21,
                                                                const char* sketch_cache_dir = nullptr) {
  std::vector<PreclusterAniMatrix> out;
  if (paths.empty()) return out;
  std::vector<const char*> c_paths;
  for (const auto& p : paths) c_paths.push_back(p.c_str());
  gg_status st = GG_OK;
  gg_ctx* ctx = gg_create_multi(kmer_length, (uint32_t)num_kmers, 0, nullptr, 0, &st);
  if (!ctx) throw std::runtime_error(std::string("Failed to sketch genomes with finch: ") + gg_thread_last_error());
  gg_set_host_threads(ctx, current_num_threads());
  uint32_t *members = nullptr, *offsets = nullptr, n_groups = 0;
  uint64_t* cells = nullptr;
  float* ani = nullptr;
  st = gg_precluster_matrices_files(ctx, c_paths.data(), (uint32_t)c_paths.size(), precluster_ani, sketch_cache_dir,
                                    &members, &offsets, &n_groups, &cells, nullptr, nullptr, &ani, nullptr);
  const std::string msg = st != GG_OK ? gg_last_error(ctx) : "";
  gg_destroy(ctx);
  if (st != GG_OK) throw std::runtime_error("Failed to sketch genomes with finch: " + msg);  // src/finch.rs:50
  out.resize(n_groups);
  for (uint32_t g = 0; g < n_groups; ++g) {
    out[g].indices.assign(members + offsets[g], members + offsets[g + 1]);
    out[g].ani.assign(ani + cells[g], ani + cells[g + 1]);
  }
  gg_free(members);
  gg_free(offsets);
  gg_free(cells);
  gg_free(ani);
  return out;
}

// src/genome_stats.rs:4-9 (#[derive(Debug, PartialEq)])
struct GenomeAssemblyStats {
  size_t num_contigs;
  size_t num_ambiguous_bases;
  size_t n50;
  bool operator==(const GenomeAssemblyStats& o) const {
    return num_contigs == o.num_contigs && num_ambiguous_bases == o.num_ambiguous_bases && n50 == o.n50;
  }
  bool operator!=(const GenomeAssemblyStats& o) const { return !(*this == o); }
};

// src/genome_stats.rs:11-51 on the host (gg_genome_stats_files); the
// reference's panic message for a file that does not read or parse
inline GenomeAssemblyStats calculate_genome_stats(const std::string& fasta_path) {
  const char* p = fasta_path.c_str();
  gg_genome_stats s{};
  if (gg_genome_stats_files(&p, 1, 1, &s) != GG_OK)
    throw std::runtime_error("Failed to calculate genome statistics for file '" + fasta_path + "': " +
                             gg_thread_last_error());
  return GenomeAssemblyStats{(size_t)s.num_contigs, (size_t)s.num_ambiguous_bases, (size_t)s.n50};
}

}  // namespace galah
