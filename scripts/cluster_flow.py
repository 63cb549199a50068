#!/usr/bin/env python3
"""Wall time of the finch + finch clustering step on the
device and on the host, same input, same process:

  device   ctx.cluster_pairs(n, pairs, ani, T)      gg_cluster_pairs: upload of the
           pairs and their ANI, the kernels, rep_of back
  host     ga.cluster_pairs_host(n, pairs, ani, T)  gg_cluster_pairs_host, one thread

Inputs: the 351 golden pairs, and synthetic cluster graphs -- genomes in
clusters (SYNTH below), a pair inside a cluster kept with a probability
that gives the wanted pair count, its ANI uniform in [0.90, 1.0) (f32) so
that about half the pairs are strong at T = 0.95, and the genome order
shuffled (galah orders by quality, not by cluster); and, as the deepest
chains of decisions a genome order can hold, the paths (i, i + 1) of 20,000
and 1,000,000 genomes with every pair strong, where each genome's decision
waits for the one before it.  Each call is timed
after one warm-up call of both, interleaved call by call; the median, the
minimum and the maximum of --steps calls are reported, with the HIP-event
time of the step's kernels and the number of representative-round launches
(from a further call).  The two results are compared on every input.
Prints one JSON line per input; --out DIR also writes them to DIR/NAME.json.

    python scripts/cluster_flow.py --steps 7 [--out profiles/cluster_flow]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import galah_amd as ga  # noqa: E402

T = np.float32(0.95)
# name: (clusters, cluster size, wanted pairs)
SYNTH = {"synth_1e5": (20, 100, 1e5), "synth_1e6": (2, 1000, 1e6), "synth_6.4e6": (2, 5000, 6.4e6)}
PATHS = {"path_2e4": 20000, "path_1e6": 1000000}


def golden_input():
    rows = []
    with open(os.path.join(ROOT, "tests", "golden", "pairs_k21_s1000.tsv")) as f:
        next(f)
        for line in f:
            i, j, _, _, a = line.split()
            rows.append((int(i), int(j), np.float32(a)))
    p = np.zeros(len(rows), ga.PAIR_DTYPE)
    p["i"], p["j"] = [r[0] for r in rows], [r[1] for r in rows]
    return 27, p, np.array([r[2] for r in rows], np.float32)


def synth_input(clusters, size, want, seed=1):
    rng = np.random.default_rng(seed)
    n = clusters * size
    order = rng.permutation(n).astype(np.uint32)  # position of each genome in the quality order
    keep = min(1.0, want / (clusters * size * (size - 1) / 2))
    ii, jj = [], []
    a, b = np.triu_indices(size, 1)
    for c in range(clusters):
        m = rng.random(len(a)) < keep
        ii.append(order[c * size + a[m]])
        jj.append(order[c * size + b[m]])
    p = np.zeros(sum(len(x) for x in ii), ga.PAIR_DTYPE)
    p["i"], p["j"] = np.concatenate(ii), np.concatenate(jj)
    ani = (np.float32(0.90) + rng.random(len(p), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    return n, p, ani


def path_input(n):
    p = np.zeros(n - 1, ga.PAIR_DTYPE)
    p["i"], p["j"] = np.arange(n - 1), np.arange(1, n)
    return n, p, np.full(n - 1, 0.97, np.float32)


def make_input(name):
    if name == "golden":
        return golden_input()
    return path_input(PATHS[name]) if name in PATHS else synth_input(*SYNTH[name])


def measure(ctx, name, n, pairs, ani, steps):
    dev = ctx.cluster_pairs(n, pairs, ani, T)  # warm-up: scratch sized, code objects loaded
    host = ga.cluster_pairs_host(n, pairs, ani, T)
    assert (dev == host).all(), name
    times = {"device": [], "host": []}
    for _ in range(steps):
        t = time.perf_counter()
        ctx.cluster_pairs(n, pairs, ani, T)  # (returns after rep_of is on the host)
        times["device"].append(time.perf_counter() - t)
        t = time.perf_counter()
        ga.cluster_pairs_host(n, pairs, ani, T)
        times["host"].append(time.perf_counter() - t)
    ctx.timing_enable(True)
    ctx.cluster_pairs(n, pairs, ani, T)
    k = ctx.timing_read(ga.KERNEL_CLUSTER)
    ctx.timing_enable(False)
    rounds = int(ctx.info_line().split("cluster round launches ")[1].split(";")[0])
    return {"input": name, "genomes": n, "pairs": int(len(pairs)), "strong_pairs": int((ani >= T).sum()),
            "clusters": int((dev == np.arange(n)).sum()), "cluster_ani": float(T), "steps": steps,
            "round_launches": rounds, "kernel_launches": int(k["launches"]), "kernel_ms": round(k["ms"], 4),
            "ms": {w: {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3),
                       "max": round(max(v) * 1e3, 3)} for w, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inputs", default="golden," + ",".join(list(SYNTH) + list(PATHS)))
    ap.add_argument("--out", help="directory for one JSON file per input")
    a = ap.parse_args()
    with ga.Context(k=21, sketch_size=1000, seed=0, device=0) as ctx:
        for name in a.inputs.split(","):
            n, pairs, ani = make_input(name)
            line = json.dumps(measure(ctx, name, n, pairs, ani, a.steps))
            print(line, flush=True)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, name + ".json"), "w") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
