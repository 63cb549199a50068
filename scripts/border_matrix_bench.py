"""Times the border form of the matrix product (gg_pairs_border_matrix_device,
DESIGN.md 4.13) against the index border (gg_pairs_border_device under the
DEFAULT pairs path: the border form of the inverted index, or of the gate kernel
where the index gives up) on the same resident rows, alternating.

Inputs: m resident rows at sketch size s in clusters of a given size, the model
rows of scripts/ani_matrix_bench.py in cluster order, the last `--new` fraction
of them new (--spread: every k-th row is moved to the end instead, so that the
new rows are members of every cluster).  Per input: a warm-up of each, then
`--calls` synchronised calls of each, alternating; the median and the spread;
the two pair lists are sorted and must be equal.  One JSON line per input, with
the counts AUTO decides from (chunk_rounds, index_reads, their ratio); --out
writes them to a file as well.

    python scripts/border_matrix_bench.py --m 10000 --clusters 5000 1000 100 10 --new 0.01 0.1
    python scripts/border_matrix_bench.py --m 100000 --clusters 10 --new 0.01

--alone runs the matrix call only, for the per-phase table from a kernel trace, one run per input:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bm -- \\
        python scripts/border_matrix_bench.py --alone --calls 1 --clusters 5000 --new 0.01

(a warm-up and one call: the per-kernel totals of DIR/**/bm_kernel_stats.csv are those of two calls).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ani_matrix_bench import model_rows  # noqa: E402
from pairs_matrix_bench import sorted_pairs  # noqa: E402


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


def alternating(fns, calls):
    """A warm-up of each, then `calls` rounds of one synchronised call of each in turn -> a stats dict per function."""
    import torch
    for fn in fns:
        fn()
        torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return [stats(x) for x in ms]


def one_input(ctx, m, s, cluster, replace, new, spread, min_ani, calls, alone, rows=None):
    import torch
    sk, lens = rows if rows is not None else model_rows(m, s, cluster, replace, seed=cluster)
    n_new = max(1, int(round(m * new)))
    n_old = m - n_new
    if spread:  # every k-th row to the end: the new rows are members of every cluster
        pick = np.arange(m)[::m // n_new][:n_new]
        keep = np.ones(m, bool)
        keep[pick] = False
        order = np.concatenate([np.flatnonzero(keep), pick])
        sk, lens = sk[order], lens[order]
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    cap = n_new * min(cluster, m) + 1024  # every pair of a new row inside its cluster, and some
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    summary = {}
    assert ctx.pairs_path == "default"

    def matrix():
        d_count.zero_()
        summary.update(ctx.pairs_border_matrix_device(d_sk, d_lens, m, n_old, min_ani, d_out, cap, d_count))

    def index():
        d_count.zero_()
        ctx.pairs_border_device(d_sk, d_lens, m, n_old, min_ani, d_out, cap, d_count)

    res = {"input": "m=%d s=%d clusters of %d, %d new%s" % (m, s, cluster, n_new, " (spread)" if spread else ""),
           "min_ani": min_ani}
    if alone:
        res["border_matrix"] = alternating([matrix], calls)[0]
        res["summary"] = dict(summary)
        return res
    before = ctx.pair_paths()
    res["border_matrix"], res["border_index"] = alternating([matrix, index], calls)
    after = ctx.pair_paths()
    res["index_paths"] = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    res["summary"] = dict(summary)
    res["ratio"] = round(summary["index_reads"] / max(summary["chunk_rounds"], 1), 1)
    # the last call was the index border's: its list against the matrix's
    n_index = int(d_count.item())
    assert n_index <= cap
    got = sorted_pairs(d_out, n_index, m).clone()
    matrix()
    torch.cuda.synchronize()
    assert int(d_count.item()) == n_index == summary["n_pairs"], (int(d_count.item()), n_index)
    assert torch.equal(sorted_pairs(d_out, n_index, m), got)
    res["pair_lists_equal"] = True
    res["n_pairs"] = n_index
    res["index_over_matrix"] = round(res["border_index"]["median_ms"] / res["border_matrix"]["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--sketch", type=int, default=1000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[5000, 1000, 100, 10], help="cluster sizes")
    ap.add_argument("--new", type=float, nargs="+", default=[0.01, 0.1], help="fractions of the rows that are new")
    ap.add_argument("--spread", action="store_true", help="the new rows drawn from every cluster, not the last rows")
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
            rows = model_rows(a.m, a.sketch, cluster, a.replace, seed=cluster)
            for new in a.new:
                res = one_input(ctx, a.m, a.sketch, cluster, a.replace, new, a.spread, min_ani, a.calls, a.alone, rows)
                print(json.dumps(res), flush=True)
                lines.append(res)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        for r in lines:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
