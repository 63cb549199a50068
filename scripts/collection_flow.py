#!/usr/bin/env python3
"""Wall time of maintaining a collection: the state kept on
the device against the state kept on the host, same process, same rows, the
two flows alternating call by call.

  add      (a) collection.add_rows_device(the last 1 % / 10 % of the rows)
           (b) the host-state flow: gg_pairs_border over host rows (every old
               sketch uploaded again), then np.concatenate + np.lexsort of the
               pair lists as FinchPreclusterer.update does them.  The border's
               ANI, which gg_update_files computes on the host, is NOT in (b)'s
               time (it is taken from the collection): (b) is favoured by that.
  cluster  (a) collection.cluster(T)
           (b) relabel_pairs on the host + gg_cluster_pairs (pairs and ANI
               uploaded), as cluster_update does
  remove   (a) collection.remove(1 % / 10 % of the rows, drawn at random)
           (b) gg_pairs over the survivors' host rows (gathered before the clock)

Inputs: the MinHash model of scripts/border_flow.py (clusters of 10, shuffled
rows) at 10k x 1000, 100k x 1000 and 10k x 10000, and "big": 10k x 1000 in 2
clusters of 5,000 (millions of pairs) for the merge and the compaction.
Each call ends in a device synchronise and is timed with the host clock after
one warm-up; median [min - max] of --steps calls.  The flows' results are
asserted equal on every input: the pair lists, their ANI where both have it,
and rep_of.  Per call the algorithmic bytes of the collection's own kernels
are reported (merge: 20 B read + 20 B written per pair of the merged list;
pair compaction: 20 B read + 8 B of flags and positions written and read per
old pair, 20 B written per survivor; row compaction: 2 x 2 x (8 s + 4) B per
moved row), not a rate: the calls' times include the border, the sort and the
clustering kernels.
Prints one JSON line per input; --out DIR also writes DIR/NAME.json.

    python scripts/collection_flow.py --steps 7 [--out profiles/collection]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import galah_amd as ga  # noqa: E402
from border_flow import synth_sketches  # noqa: E402

MIN_ANI = np.float32(0.95)
CLUSTER_ANI = np.float32(0.97)
K = 21
# name: (rows, sketch size, (smallest, largest) genome length in k-mers, cluster size)
INPUTS = {"c3_10k": (10000, 1000, (3e6, 3e6), 10), "c3_100k": (100000, 1000, (3e6, 3e6), 10),
          "c5_10k": (10000, 10000, (0.5e6, 12e6), 10), "big": (10000, 1000, (3e6, 3e6), 5000)}
SHARES = {"1pct": 0.01, "10pct": 0.10}


def stats(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}


def clock(f):
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def same_pairs(a, b):
    return a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


def measure(ctx, name, steps):
    n, s, lengths, cluster = INPUTS[name]
    d_sk, d_lens = synth_sketches(n, s, lengths, cluster=cluster)
    h_sk = d_sk.cpu().numpy().view(np.uint64)
    h_lens = d_lens.cpu().numpy().view(np.uint32)
    thr, T = float(MIN_ANI), float(CLUSTER_ANI)
    out = {"input": name, "rows": n, "sketch_size": s, "cluster_size": cluster, "min_ani": thr, "cluster_ani": T,
           "steps": steps, "add": {}, "cluster": {}, "remove": {}}
    row = 8 * s + 4
    for what, share in SHARES.items():
        n_new = max(1, int(round(n * share)))
        n_old = n - n_new
        h = ctx.collection_create(thr, n, 0)
        try:
            ctx.collection_add_rows_device(h, d_sk, d_lens, n_old)
            old_pairs, old_ani = ctx.collection_pairs(h)
            new_rows = np.arange(n_old, n, dtype=np.uint32)
            t = {"add_a": [], "add_b": [], "cluster_a": [], "cluster_b": []}
            for step in range(steps + 1):  # (the first round warms both flows up)
                ta, added = clock(lambda: ctx.collection_add_rows_device(h, d_sk[n_old:], d_lens[n_old:], n_new))
                tca, rep_a = clock(lambda: ctx.collection_cluster(h, T))
                all_pairs, all_ani = ctx.collection_pairs(h)

                def host_add():
                    border = ctx.pairs_border(h_sk, h_lens, n_old, thr)
                    pairs = np.concatenate([old_pairs, border])
                    by_ij = np.lexsort((pairs["j"], pairs["i"]))
                    return pairs[by_ij], by_ij
                tb, (pairs_b, by_ij) = clock(host_add)
                assert same_pairs(pairs_b, all_pairs), (name, what, "pairs")
                border_ani = all_ani[all_pairs["j"] >= n_old]
                ani_b = np.concatenate([old_ani, border_ani])[by_ij]
                assert (ani_b.view(np.uint32) == all_ani.view(np.uint32)).all(), (name, what, "ani")
                tcb, rep_b = clock(lambda: ctx.cluster_pairs(n, ga.relabel_pairs(pairs_b, np.arange(n)), ani_b, T))
                assert (rep_a == rep_b).all(), (name, what, "rep_of")
                ctx.collection_remove(h, new_rows)  # back to the old rows (the last rows: nothing moves)
                if step:
                    for key, v in (("add_a", ta), ("add_b", tb), ("cluster_a", tca), ("cluster_b", tcb)):
                        t[key].append(v)
            out["add"][what] = {"new_rows": n_new, "pairs_before": len(old_pairs), "pairs_added": int(added),
                                "collection_ms": stats(t["add_a"]), "host_state_ms": stats(t["add_b"]),
                                "merge_bytes": 40 * len(all_pairs)}
            out["cluster"][what] = {"pairs": len(all_pairs), "collection_ms": stats(t["cluster_a"]),
                                    "host_state_ms": stats(t["cluster_b"])}
            # removal: the whole set, rows drawn at random, put back (at the end) after each call
            ctx.collection_add_rows_device(h, d_sk[n_old:], d_lens[n_old:], n_new)
            ids = np.arange(n)  # the original row held at each index
            rng = np.random.default_rng(11)
            t = {"a": [], "b": []}
            moved = kept_pairs = 0
            for step in range(steps + 1):
                n_pairs_before = ctx.collection_stat(h)[0]["n_pairs"]
                gone = np.sort(rng.choice(n, n_new, replace=False)).astype(np.uint32)
                ta, new_index = clock(lambda: ctx.collection_remove(h, gone))
                moved = ctx.collection_stat(h)[0]["rows_moved"]
                keep = new_index != 0xFFFFFFFF
                surv = ids[keep]
                sk_keep, lens_keep = h_sk[surv], h_lens[surv]
                tb, pairs_b = clock(lambda: ctx.pairs(sk_keep, lens_keep, thr))
                pairs_a, _ = ctx.collection_pairs(h)
                assert same_pairs(pairs_a, pairs_b), (name, what, "pairs after removal")
                kept_pairs = len(pairs_a)
                back = torch.from_numpy(ids[~keep]).cuda()
                ctx.collection_add_rows_device(h, d_sk[back].contiguous(), d_lens[back].contiguous(), n_new)
                ids = np.concatenate([surv, ids[~keep]])
                if step:
                    t["a"].append(ta)
                    t["b"].append(tb)
            out["remove"][what] = {"rows_removed": n_new, "rows_moved_last": int(moved), "pairs_before": int(n_pairs_before),
                                   "pairs_kept_last": int(kept_pairs), "collection_ms": stats(t["a"]),
                                   "pairs_from_scratch_ms": stats(t["b"]),
                                   "pair_compaction_bytes": 36 * int(n_pairs_before) + 20 * int(kept_pairs),
                                   "row_compaction_bytes": 4 * row * int(moved)}
            out["device_bytes"] = ctx.collection_stat(h)[0]["device_bytes"]
        finally:
            ctx.collection_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--out", help="directory for one JSON file per input")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "collection_flow.py needs a GPU"
    for name in a.inputs.split(","):
        with ga.Context(k=K, sketch_size=INPUTS[name][1], seed=0, device=0) as ctx:
            line = json.dumps(measure(ctx, name, a.steps))
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name + ".json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
