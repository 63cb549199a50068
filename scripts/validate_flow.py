#!/usr/bin/env python3
"""Wall time of the named-pair ANI call and of cluster validation (DESIGN.md
4.6) on the device and on the host, same input, same process:

  named pairs   ctx.ani_pairs(sk, lens, list)       gg_ani_pairs: upload of the sketch
                matrix and the list, one kernel, the list back, the f32 on the host
                ga.ani_pairs_host(sk, lens, list)   gg_ani_pairs_host: finch's merge, one thread
  validation    ctx.validate_clusters(...)          gg_validate_clusters
                ga.validate_clusters_host(...)      gg_validate_clusters_host, one thread

Named pairs: the 351 golden pairs, and 1e4 / 1e5 / 1e6 random pairs over
synthetic sketches -- 2,000 rows at s = 1000 (every row fits the kernel's LDS
slice) and 300 rows at s = 10000 (rows searched in global memory), each row a
draw of s hashes from a pool of 2 s, so two rows share about half -- once
grouped by i and once shuffled.  Validation: "20x100", 20 clusters of 100
genomes, and "2000+8000", 2,000 representatives with 8,000 members between
them; a cluster's rows are draws from the cluster's own pool of 1.5 s hashes
(ANI ~0.98 inside a cluster, 0 between clusters), threshold 0.95.

Each call is timed after one warm-up call of both, interleaved call by call;
the median, the minimum and the maximum of --steps calls are reported, with
the HIP-event time of the named-pair kernel (from a further call).  The host
calls of an input are cut short when they would take more than --host-budget
seconds together (the line's "host_steps" says how many were timed; the
warm-up call is the one timed when a single call exceeds the budget), and
the host form is not timed at all where one call would take minutes (1e6
pairs at s = 10000: "host_steps" 0, the device result compared with the host
form on a sample of 20,000 entries).  Otherwise the two results are compared
whole on every input.  Prints one JSON line per input; --out
DIR also writes them to DIR/NAME.json.

    python scripts/validate_flow.py --steps 7 [--out profiles/validate_flow]
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
ROWS = {1000: 2000, 10000: 300}  # sketch size: rows of the synthetic matrix
COUNTS = {"1e4": 10000, "1e5": 100000, "1e6": 1000000}
HOST_MAX_STEPS = 4e9  # pairs x sketch size above which the host form is not timed (~7 ns per merge step)
VALIDATE = {"validate_20x100": (20, 99), "validate_2000+8000": (2000, 4)}  # clusters, members per cluster


def rows_from_pool(rng, pool, count, s):
    return np.sort(np.stack([rng.choice(pool, size=s, replace=False) for _ in range(count)]), axis=1)


def pool_of(rng, size):
    p = np.unique(rng.integers(1, 1 << 63, size=size + size // 8 + 16, dtype=np.uint64))
    return rng.permutation(p)[:size]


def golden_input():
    with np.load(os.path.join(ROOT, "tests", "golden", "sketches_k21_s1000.npz")) as z:
        sk, lens = z["sketches"].copy(), z["lens"].copy()
    pairs = np.array([(i, j) for i in range(27) for j in range(i + 1, 27)], dtype=np.uint32)
    return sk, lens, pairs


def pairs_input(s, m, order, seed=1):
    rng = np.random.default_rng(seed + s)
    n = ROWS[s]
    sk = rows_from_pool(rng, pool_of(rng, 2 * s), n, s)
    pairs = rng.integers(0, n, size=(m, 2), dtype=np.uint32)
    if order == "grouped":
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return sk, np.full(n, s, dtype=np.uint32), pairs


def validate_input(clusters, members, s=1000, seed=5):
    rng = np.random.default_rng(seed)
    rows, out = [], []
    for c in range(clusters):
        first = c * (members + 1)
        rows.append(rows_from_pool(rng, pool_of(rng, s + s // 2), members + 1, s))
        out.append(list(range(first, first + members + 1)))
    sk = np.concatenate(rows)
    return sk, np.full(len(sk), s, dtype=np.uint32), out


def summary(times):
    return {w: {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3),
                "max": round(max(v) * 1e3, 3)} for w, v in times.items()}


def timed(f):
    t = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t


def interleaved(device, host, steps, host_budget):
    """Warm-up of both (compared by the caller), then the timed calls."""
    dev, _ = timed(device)
    hst, first_host = timed(host)
    host_steps = steps if first_host * steps <= host_budget else int(host_budget / first_host)
    times = {"device": [], "host": [] if host_steps else [first_host]}
    for x in range(steps):
        times["device"].append(timed(device)[1])
        if x < host_steps:
            times["host"].append(timed(host)[1])
    return dev, hst, times, max(host_steps, 1)


def measure_pairs(ctx, name, sk, lens, pairs, steps, host_budget):
    m, s = len(pairs), sk.shape[1]
    if m * s <= HOST_MAX_STEPS:
        (dev, dev_ani), (hst, hst_ani), times, host_steps = interleaved(
            lambda: ctx.ani_pairs(sk, lens, pairs), lambda: ga.ani_pairs_host(sk, lens, pairs, k=ctx.k), steps,
            host_budget)
        assert dev.tobytes() == hst.tobytes() and dev_ani.tobytes() == hst_ani.tobytes(), name
    else:  # the host form is not timed (minutes per call): the device result is checked on a sample
        sample = np.sort(np.random.default_rng(9).choice(m, size=20000, replace=False))
        dev, dev_ani = ctx.ani_pairs(sk, lens, pairs)
        hst, hst_ani = ga.ani_pairs_host(sk, lens, pairs[sample], k=ctx.k)
        assert dev[sample].tobytes() == hst.tobytes() and dev_ani[sample].tobytes() == hst_ani.tobytes(), name
        times, host_steps = {"device": [timed(lambda: ctx.ani_pairs(sk, lens, pairs))[1] for _ in range(steps)]}, 0
    def kernel_ms():
        ctx.timing_enable(True)
        ctx.ani_pairs(sk, lens, pairs)
        k = ctx.timing_read(ga.KERNEL_ANI_PAIRS)
        ctx.timing_enable(False)
        assert k["launches"] == 1 and k["work"] == m
        return round(k["ms"], 4)

    out = {"input": name, "genomes": int(len(lens)), "sketch_size": int(s), "pairs": int(m),
           "path": "lds" if s <= 2048 else "global", "steps": steps, "host_steps": host_steps,
           "kernel_ms": kernel_ms()}
    if s <= 2048:  # the same rows left in global memory (GALAHGPU_ANI_PAIRS_LDS=0)
        os.environ["GALAHGPU_ANI_PAIRS_LDS"] = "0"
        try:
            alt, _ = ctx.ani_pairs(sk, lens, pairs)
            assert alt.tobytes() == dev.tobytes(), name
            times["device_global"] = [timed(lambda: ctx.ani_pairs(sk, lens, pairs))[1] for _ in range(steps)]
            out["kernel_ms_global"] = kernel_ms()
        finally:
            del os.environ["GALAHGPU_ANI_PAIRS_LDS"]
    out["ms"] = summary(times)
    return out


def measure_validate(ctx, name, sk, lens, clusters, steps, host_budget):
    dev, hst, times, host_steps = interleaved(
        lambda: ctx.validate_clusters(sk, lens, clusters, T),
        lambda: ga.validate_clusters_host(sk, lens, clusters, T, k=ctx.k), steps, host_budget)
    assert dev.bad.tobytes() == hst.bad.tobytes() and dev.bad_ani.tobytes() == hst.bad_ani.tobytes(), name
    assert (dev.member_pairs, dev.rep_pairs) == (hst.member_pairs, hst.rep_pairs), name
    ctx.timing_enable(True)
    ctx.validate_clusters(sk, lens, clusters, T)
    k = ctx.timing_read(ga.KERNEL_ANI_PAIRS)
    k2 = ctx.timing_read(ga.KERNEL_PAIRS)
    ki = ctx.timing_read(ga.KERNEL_PAIRS_INDEX)
    ctx.timing_enable(False)
    return {"input": name, "genomes": int(len(lens)), "sketch_size": int(sk.shape[1]), "clusters": len(clusters),
            "member_pairs": dev.member_pairs, "member_bad": dev.member_bad, "rep_pairs": dev.rep_pairs,
            "rep_bad": dev.rep_bad, "threshold": float(T), "steps": steps, "host_steps": host_steps,
            "named_kernel_ms": round(k["ms"], 4), "pair_kernels_ms": round(k2["ms"] + ki["ms"], 4),
            "ms": summary(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-budget", type=float, default=20.0, help="seconds of timed host calls per input")
    names = ["golden_351"] + ["pairs_s%d_%s_%s" % (s, c, o) for s in ROWS for c in COUNTS
                              for o in ("grouped", "shuffled")]
    ap.add_argument("--inputs", default=",".join(names + list(VALIDATE)))
    ap.add_argument("--out", help="directory for one JSON file per input")
    a = ap.parse_args()
    ctxs = {}
    try:
        for name in a.inputs.split(","):
            if name in VALIDATE:
                sk, lens, clusters = validate_input(*VALIDATE[name])
            elif name == "golden_351":
                sk, lens, pairs = golden_input()
            else:
                _, s, count, order = name.split("_")
                sk, lens, pairs = pairs_input(int(s[1:]), COUNTS[count], order)
            s = sk.shape[1]
            if s not in ctxs:
                ctxs[s] = ga.Context(k=21, sketch_size=s, seed=0, device=0)
            if name in VALIDATE:
                res = measure_validate(ctxs[s], name, sk, lens, clusters, a.steps, a.host_budget)
            else:
                res = measure_pairs(ctxs[s], name, sk, lens, pairs, a.steps, a.host_budget)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, name + ".json"), "w") as f:
                    f.write(line + "\n")
    finally:
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    main()
