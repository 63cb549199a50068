// Host runtime of the finch + finch clustering step: what
// galah's cluster() does after the preclusters when the clusterer reuses the
// preclusterer's ANI values (src/clusterer.rs:29-33, :180-185).
//
//   src/clusterer.rs:155-225  representatives: per genome i, a scan of the
//     representatives so far -- O(N * reps) cache lookups;
//   src/clusterer.rs:316-406  memberships: per non-representative, a scan of
//     all representatives.
//
// Here both walk the adjacency of the sparse pair list (one counting sort):
// linear in the pairs.  The rules themselves are cluster_core.hpp's, shared
// with the kernels (cluster.hip); this form is the entry point of callers
// without a context and the CPU-testable twin of the device path.
//
// Preclusters do not enter: they are the connected components of the same
// pairs and keep their members in input order, so the two loops run per
// precluster (:66-123) decide exactly what they decide over the whole list.
//
// Order of the clusters (gg_clusters_from_reps): by representative
// ascending, the representative first, then its members ascending.  The
// reference pushes each precluster's clusters in rayon completion order
// (:114-121) and its members as a parallel loop reaches them (:341-401), so
// no output of galah depends on it.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "cluster_core.hpp"
#include "gg_internal.hpp"

namespace gg {

// The checks of the host-input forms (gg_cluster_pairs_host, gg_cluster_pairs).
gg_status cluster_check_input(const char* who, uint32_t n_genomes, const gg_pair* pairs, const float* ani,
                              uint64_t n_pairs, float cluster_ani, const uint32_t* rep_of) {
  const std::string w(who);
  if ((n_pairs && (!pairs || !ani)) || (n_genomes && !rep_of)) {
    set_thread_error(w + ": null argument");
    return GG_ERR_INVALID_ARG;
  }
  if (std::isnan(cluster_ani)) {
    set_thread_error(w + ": cluster_ani is NaN");
    return GG_ERR_INVALID_ARG;
  }
  if (n_pairs >= (1ull << 31)) {
    set_thread_error(w + ": 2^31 pairs or more");
    return GG_ERR_INVALID_ARG;
  }
  for (uint64_t p = 0; p < n_pairs; ++p) {
    if (pairs[p].i >= n_genomes || pairs[p].j >= n_genomes) {
      set_thread_error(w + ": pair index out of range");
      return GG_ERR_INVALID_ARG;
    }
    if (pairs[p].i == pairs[p].j) {
      set_thread_error(w + ": pair of a genome with itself");
      return GG_ERR_INVALID_ARG;
    }
    if (std::isnan(ani[p])) {
      set_thread_error(w + ": NaN ani");
      return GG_ERR_INVALID_ARG;
    }
  }
  return GG_OK;
}

}  // namespace gg

using namespace gg;

extern "C" gg_status gg_cluster_pairs_host(uint32_t n_genomes, const gg_pair* pairs, const float* ani,
                                           uint64_t n_pairs, float cluster_ani, uint32_t* rep_of) {
  const gg_status st = cluster_check_input("gg_cluster_pairs_host", n_genomes, pairs, ani, n_pairs, cluster_ani, rep_of);
  if (st != GG_OK) return st;
  const uint32_t n = n_genomes;
  // adjacency, both directions, each edge with its pair
  std::vector<uint32_t> off((size_t)n + 1, 0);
  for (uint64_t p = 0; p < n_pairs; ++p) {
    ++off[pairs[p].i + 1];
    ++off[pairs[p].j + 1];
  }
  for (uint32_t v = 0; v < n; ++v) off[v + 1] += off[v];
  std::vector<uint32_t> nbr(2 * n_pairs), src(2 * n_pairs), fill(off.begin(), off.end() - 1);
  for (uint64_t p = 0; p < n_pairs; ++p) {
    const uint32_t i = pairs[p].i, j = pairs[p].j;
    nbr[fill[i]] = j;
    src[fill[i]++] = (uint32_t)p;
    nbr[fill[j]] = i;
    src[fill[j]++] = (uint32_t)p;
  }
  // representatives: ascending, so every lower vertex is decided
  std::vector<uint32_t> state(n, cluster::kUndecided);
  for (uint32_t v = 0; v < n; ++v) {
    cluster::Seen seen;
    for (uint32_t e = off[v]; e < off[v + 1]; ++e)
      if (nbr[e] < v && cluster::strong(ani[src[e]], cluster_ani)) cluster::see(seen, state[nbr[e]]);
    state[v] = cluster::decide(seen);
  }
  // memberships
  for (uint32_t v = 0; v < n; ++v) {
    if (state[v] == cluster::kRep) {
      rep_of[v] = v;
      continue;
    }
    uint64_t best = 0;
    for (uint32_t e = off[v]; e < off[v + 1]; ++e)
      if (state[nbr[e]] == cluster::kRep) best = std::max(best, cluster::member_key(ani[src[e]], nbr[e]));
    rep_of[v] = cluster::key_rep(best);  // (a member has a strong representative neighbour: best != 0)
  }
  return GG_OK;
}

extern "C" gg_status gg_clusters_from_reps(uint32_t n_genomes, const uint32_t* rep_of, uint32_t* members,
                                           uint32_t* offsets, uint32_t* n_clusters) {
  if ((n_genomes && (!rep_of || !members)) || !offsets || !n_clusters) {
    set_thread_error("gg_clusters_from_reps: null argument");
    return GG_ERR_INVALID_ARG;
  }
  const uint32_t n = n_genomes;
  *n_clusters = 0;
  offsets[0] = 0;
  for (uint32_t g = 0; g < n; ++g) {
    if (rep_of[g] >= n || rep_of[rep_of[g]] != rep_of[g]) {
      set_thread_error("gg_clusters_from_reps: rep_of does not point at representatives");
      return GG_ERR_INVALID_ARG;
    }
  }
  // cluster sizes by representative, then the representatives numbered ascending
  std::vector<uint32_t> size(n, 0), at(n, 0);
  for (uint32_t g = 0; g < n; ++g) ++size[rep_of[g]];
  uint32_t nc = 0, pos = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (rep_of[r] != r) continue;
    members[pos] = r;  // the representative first
    at[r] = pos + 1;
    pos += size[r];
    offsets[++nc] = pos;
  }
  for (uint32_t g = 0; g < n; ++g)
    if (rep_of[g] != g) members[at[rep_of[g]]++] = g;  // ascending
  *n_clusters = nc;
  return GG_OK;
}
