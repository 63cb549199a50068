"""The reference's two clustering loops, restated in Python for the finch +
finch mode (skip_clusterer = true, src/clusterer.rs:29-33), with a clusterer
whose value for a pair is the cached one.  A test helper, deliberately in the
reference's own structure -- per genome, a scan of the current representative
set -- so that it shares nothing with the library's adjacency walk.

  find_representatives   src/clusterer.rs:155-225
  find_memberships       src/clusterer.rs:316-406
  cluster_ref            both, over the whole pair cache -> rep_of

There is no reference output for this mode (galah's CLUSTER_METHODS has no
finch): the library is pinned to this restatement.
"""
import numpy as np


def make_cache(pairs, ani):
    """SortedPairGenomeDistanceCache: {(min, max): f32}."""
    cache = {}
    for (i, j), a in zip(pairs, ani):
        i, j = int(i), int(j)
        cache[(i, j) if i < j else (j, i)] = np.float32(a)
    return cache


def _get(cache, a, b):
    return cache.get((a, b) if a < b else (b, a))


def find_representatives(n, cache, threshold):
    """:155-225 with skip_clusterer: compute_ani_from_preclusterer (:264-279)
    returns the cached values of the representatives that have one."""
    threshold = np.float32(threshold)
    reps = []  # BTreeSet<usize>: genomes are visited ascending, so appending keeps it sorted
    for i in range(n):
        # :167-177 -- the representatives with a cached pair, sorted by ANI
        found = [(j, _get(cache, i, j)) for j in reps]
        found = [(j, a) for j, a in found if a is not None]
        found.sort(key=lambda x: x[1])
        is_rep = True
        for _, a in found:
            if a >= threshold:  # :212
                is_rep = False
        if is_rep:
            reps.append(i)
    return reps


def find_memberships(n, reps, cache):
    """:316-406 -> rep_of.  Every (i, rep) pair of the precluster cache ends
    up in calculated_fastanis with the clusterer's value, here the cached one
    (:343-371), so the scan of :376-399 reads the cache."""
    rep_set = set(reps)
    rep_of = np.zeros(n, np.uint32)
    for i in range(n):
        if i in rep_set:
            rep_of[i] = i
            continue
        best_rep, best = None, None
        for rep in reps:  # BTreeSet iteration: ascending
            a = _get(cache, i, rep)
            if a is not None and (best is None or a > best):  # :394-399, strict
                best_rep, best = rep, a
        rep_of[i] = best_rep  # best_rep.unwrap()
    return rep_of


def cluster_ref(n, pairs, ani, threshold):
    cache = make_cache(pairs, ani)
    return find_memberships(n, find_representatives(n, cache, threshold), cache)


def clusters_ref(rep_of):
    """Clusters by representative ascending, the representative first, then
    the members ascending."""
    out = {}
    for g, r in enumerate(rep_of):
        out.setdefault(int(r), [])
    for g, r in enumerate(rep_of):
        if int(r) != g:
            out[int(r)].append(g)
    return [[r] + out[r] for r in sorted(out)]
