#!/usr/bin/env python3
"""Writes tests/golden/clusters_finch.tsv: the finch + finch clusters of the
27 golden genomes, as rep_of rows, from the committed pair table
(pairs_k21_s1000.tsv: all 351 pairs with the f32 ANI galah stores).

galah has no output for this mode (its CLUSTER_METHODS has no finch), so the
rows come from the restatement of the reference's two loops
(src/clusterer.rs:155-225 and :316-406 with skip_clusterer) in
tests/cluster_ref.py, independent of the library.  One row per (precluster
ANI, cluster ANI): the pairs with ANI >= the precluster ANI are the cache.
The script checks the cluster counts (5, 5, 7, 10, 16, 21 at either
precluster ANI) and the number of members whose representative has a higher
index (0, 0, 1, 5, 1, 0) before it writes anything.

    python tests/golden/make_clusters_finch.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cluster_ref import cluster_ref  # noqa: E402

MIN_ANI = ("0.9", "0.0")
CLUSTER_ANI = ("0.9", "0.95", "0.97", "0.98", "0.99", "0.995")
N_CLUSTERS = (5, 5, 7, 10, 16, 21)
N_BACKWARD = (0, 0, 1, 5, 1, 0)


def main():
    rows = []
    with open(os.path.join(HERE, "pairs_k21_s1000.tsv")) as f:
        next(f)
        for line in f:
            i, j, _, _, a = line.split()
            rows.append((int(i), int(j), np.float32(a)))
    assert len(rows) == 351
    out = []
    for m in MIN_ANI:
        kept = [r for r in rows if np.float64(r[2]) >= np.float64(np.float32(m))]
        assert len(kept) == (161 if m == "0.9" else 351)
        for t, nc, nb in zip(CLUSTER_ANI, N_CLUSTERS, N_BACKWARD):
            rep_of = cluster_ref(27, [(i, j) for i, j, _ in kept], [a for _, _, a in kept], np.float32(t))
            assert len(set(rep_of.tolist())) == nc, (m, t, len(set(rep_of.tolist())))
            assert sum(int(r) > g for g, r in enumerate(rep_of)) == nb, (m, t)
            out.append((m, t, ",".join(str(int(r)) for r in rep_of)))
    with open(os.path.join(HERE, "clusters_finch.tsv"), "w") as f:
        f.write("min_ani\tcluster_ani\trep_of\n")
        for r in out:
            f.write("%s\t%s\t%s\n" % r)
    print("wrote %d rows" % len(out))


if __name__ == "__main__":
    main()
