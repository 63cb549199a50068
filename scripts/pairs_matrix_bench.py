"""Times the pair form of the matrix product (gg_pairs_matrix_device, DESIGN.md
4.12) against K2 (gg_pairs_device over every tile: the inverted index, or the
gate kernel where the index gives up) on the same resident rows, and
gg_cluster_rows_device under the three pairs paths.

Inputs: m resident rows at sketch size s in clusters of a given size, the
model rows of scripts/ani_matrix_bench.py (a base of s random hashes per
cluster, each member replacing a fraction by hashes of its own).  Per input: a
warm-up call, then the median and the spread of `--calls` synchronised calls
of each of the five; the two pair lists are sorted and must be equal.  One
JSON line per input, with the counts AUTO decides from (chunk_rounds,
index_reads, their ratio); --out writes them to a file as well.

    python scripts/pairs_matrix_bench.py --m 10000 --clusters 10 100 1000 5000
    python scripts/pairs_matrix_bench.py --m 100000 --clusters 10   # (2.4e10 chunk rounds: minutes a call)

--alone runs the matrix call only, for the per-phase table from a kernel trace, one run per input:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pm -- \\
        python scripts/pairs_matrix_bench.py --alone --calls 1 --clusters 1000

(a warm-up and one call: the per-kernel totals of DIR/**/pm_kernel_stats.csv are those of two calls).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ani_matrix_bench import model_rows, timed  # noqa: E402


def sorted_pairs(d_pairs, n, m):
    """The first n records of an int32 [cap, 4] tensor in (i, j) order."""
    import torch
    p = d_pairs[:n]
    key = (p[:, 0].long() & 0xFFFFFFFF) * m + (p[:, 1].long() & 0xFFFFFFFF)
    return p[torch.argsort(key)]


def one_input(ctx, ga, m, s, cluster, replace, min_ani, calls, alone):
    import torch
    sk, lens = model_rows(m, s, cluster, replace, seed=cluster)
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    cap = m * (cluster - 1) // 2 + 1024  # every pair inside a cluster, and some
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_rep = torch.zeros(m, dtype=torch.int32, device="cuda")
    summary = {}

    def matrix():
        d_count.zero_()
        summary.update(ctx.pairs_matrix_device(d_sk, d_lens, m, None, m, min_ani, d_out, cap, d_count))

    res = {"input": "m=%d s=%d clusters of %d" % (m, s, cluster), "min_ani": min_ani}
    res["pairs_matrix"] = timed(matrix, calls)
    n_matrix = int(d_count.item())
    res["summary"] = dict(summary)
    res["ratio"] = round(summary["index_reads"] / max(summary["chunk_rounds"], 1), 1)
    if alone:
        return res
    assert n_matrix <= cap
    got = sorted_pairs(d_out, n_matrix, m).clone()

    def k2():
        d_count.zero_()
        ctx.pairs_device(d_sk, d_lens, m, 0, ga.pair_tiles(m), min_ani, d_out, cap, d_count)

    before = ctx.pair_paths()
    res["pairs_k2"] = timed(k2, calls)
    after = ctx.pair_paths()
    res["k2_paths"] = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert int(d_count.item()) == n_matrix, (int(d_count.item()), n_matrix)
    assert torch.equal(sorted_pairs(d_out, n_matrix, m), got)
    res["pair_lists_equal"] = True
    res["n_pairs"] = n_matrix
    res["k2_over_matrix"] = round(res["pairs_k2"]["median_ms"] / res["pairs_matrix"]["median_ms"], 2)
    del got

    reps = {}
    for path in ga.PAIRS_PATHS:
        ctx.set_pairs_path(path)
        taken = ctx.pairs_paths_taken()
        res["cluster_rows_" + path] = timed(
            lambda: ctx.cluster_rows_device(d_sk, d_lens, m, min_ani, min_ani, d_rep, want_summary=False), calls)
        now = ctx.pairs_paths_taken()
        res["cluster_rows_" + path]["ran"] = [k for k in now if now[k] != taken[k]]
        reps[path] = d_rep.clone()
    ctx.set_pairs_path("default")
    assert torch.equal(reps["matrix"], reps["default"]) and torch.equal(reps["auto"], reps["default"])
    res["rep_of_equal"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--sketch", type=int, default=1000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[10, 100, 1000, 5000], help="cluster sizes, one input each")
    ap.add_argument("--replace", type=float, default=0.05, help="fraction of a member's hashes that are its own")
    ap.add_argument("--min-ani", type=float, default=0.95)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--alone", action="store_true", help="the matrix call only, nothing to compare with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import galah_amd as ga

    min_ani = float(np.float32(a.min_ani))
    lines = []
    with ga.Context(k=21, sketch_size=a.sketch, seed=0, device=0) as ctx:
        for cluster in a.clusters:
            res = one_input(ctx, ga, a.m, a.sketch, cluster, a.replace, min_ani, a.calls, a.alone)
            print(json.dumps(res), flush=True)
            lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
