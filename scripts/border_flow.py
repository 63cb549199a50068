#!/usr/bin/env python3
"""Wall time of adding genomes to a finished run: the border
call over the new rows against the all-pairs call over the same rows, same
process, same device-resident sketch matrix:

  border   ctx.pairs_border_device(d_sk, d_lens, n, n_old, ...)  the last 1 % and
           the last 10 % of the rows as the new ones
  full     ctx.pairs_device(d_sk, d_lens, n, 0, all tiles, ...)   what an update
           costs without the border form

Inputs: sketches made on the device from a MinHash model of BASELINE's
synthetic sets -- genomes in clusters of 10, a member keeps each of its
cluster's k-mers with probability (1 - r)^21 for a substitution rate r drawn
in [0, 0.07) and holds fresh k-mers in their place; a sketch is the bottom s
of the 2 s smallest hashes so made, which lie uniformly below 2 s / L x 2^64
for a genome of L k-mers.  c3_10k / c3_100k: L = 3e6, s = 1000; c5_10k:
L log-uniform in 0.5e6 .. 12e6 per cluster, s = 10000.  The row order is
shuffled, so that new rows belong to clusters of old rows.

Each call ends in a device synchronise and is timed with the host clock
after one warm-up call of each, the three calls alternating step by step;
the median, minimum and maximum of --steps calls are reported, then the
HIP-event time of each call's kernels by phase (gg_timing_read: the index
build, the pairs kernel) from one further call, and which K2 form ran.  The
border's pairs are compared with the full call's pairs of the same columns
on every input.  --full-only times the full call alone: it runs with an
older library (GALAHGPU_LIB) too, for the unchanged-path comparison.
Prints one JSON line per input; --out DIR also writes DIR/NAME[_TAG].json.

    python scripts/border_flow.py --steps 15 [--out profiles/border]
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

MIN_ANI = np.float32(0.95)
CLUSTER, MAX_SUB, K = 10, 0.07, 21
# name: (rows, sketch size, (smallest, largest) genome length in k-mers)
INPUTS = {"c3_10k": (10000, 1000, (3e6, 3e6)), "c3_100k": (100000, 1000, (3e6, 3e6)),
          "c5_10k": (10000, 10000, (0.5e6, 12e6))}
NEW_SHARES = {"border_1pct": 0.01, "border_10pct": 0.10}


def synth_sketches(n, s, lengths, seed=5, device="cuda", cluster=CLUSTER):
    """-> (d_sk [n, s] int64 holding the u64 hashes, ascending; d_lens [n] int32); cluster: genomes per cluster."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    clusters = (n + cluster - 1) // cluster
    lo, hi = lengths
    length = lo * (hi / lo) ** torch.rand(clusters, generator=g, device=device, dtype=torch.float64)
    bound = (2.0 * s / length * 2.0 ** 64).to(torch.int64)  # (below 2^63: 2 s < L / 2)
    out = torch.empty((clusters * cluster, s), dtype=torch.int64, device=device)
    step = max(1, (1 << 24) // (cluster * 2 * s))  # clusters per chunk: ~128 MB of candidates
    for c0 in range(0, clusters, step):
        c1 = min(clusters, c0 + step)
        b = bound[c0:c1].to(torch.float64).view(-1, 1, 1)
        draw = lambda *shape: (torch.rand(*shape, generator=g, device=device, dtype=torch.float64) * b).to(torch.int64)
        base = draw(c1 - c0, 1, 2 * s)
        rate = MAX_SUB * torch.rand((c1 - c0, cluster, 1), generator=g, device=device, dtype=torch.float64)
        keep = torch.rand((c1 - c0, cluster, 2 * s), generator=g, device=device, dtype=torch.float64) < (1 - rate) ** K
        member = torch.where(keep, base.expand(-1, cluster, -1), draw(c1 - c0, cluster, 2 * s))
        member = torch.sort(member, dim=2).values[:, :, :s]
        out[c0 * cluster:c1 * cluster] = member.reshape(-1, s)
    assert bool((out[:, 1:] > out[:, :-1]).all()), "a repeated hash in a synthetic sketch"
    rows = torch.randperm(clusters * cluster, generator=g, device=device)[:n]
    return out[rows].contiguous(), torch.full((n,), s, dtype=torch.int32, device=device)


def sorted_quads(buf, count):
    q = buf[:count * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
    return q[np.lexsort((q[:, 1], q[:, 0]))]


def stats(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}


def measure(ctx, name, steps, full_only):
    n, s, lengths = INPUTS[name]
    d_sk, d_lens = synth_sketches(n, s, lengths)
    cap = 64 * n
    d_out = torch.empty((cap * 4,), dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    tiles = ga.pair_tiles(n)

    def full():
        d_cnt.zero_()
        ctx.pairs_device(d_sk, d_lens, n, 0, tiles, MIN_ANI, d_out, cap, d_cnt)
        torch.cuda.synchronize()

    def border(n_old):
        d_cnt.zero_()
        ctx.pairs_border_device(d_sk, d_lens, n, n_old, MIN_ANI, d_out, cap, d_cnt)
        torch.cuda.synchronize()

    calls = {"full": full}
    n_old = {}
    if not full_only:
        for what, share in NEW_SHARES.items():
            n_old[what] = n - max(1, int(round(n * share)))
            calls[what] = (lambda m: lambda: border(m))(n_old[what])
    # warm-up, and the border against the full call's pairs of the same columns
    full()
    m_full = int(d_cnt.item())
    assert m_full <= cap
    q_full = sorted_quads(d_out, m_full)
    pairs = {"full": m_full}
    for what in n_old:
        calls[what]()
        m = int(d_cnt.item())
        exp = q_full[q_full[:, 1] >= n_old[what]]
        got = sorted_quads(d_out, m)
        assert got.shape == exp.shape and (got == exp).all(), (name, what)
        pairs[what] = m
    times = {what: [] for what in calls}
    for _ in range(steps):
        for what, call in calls.items():
            t = time.perf_counter()
            call()
            times[what].append(time.perf_counter() - t)
    # HIP-event time of each call's kernels by phase, and the K2 form that ran
    kernel_ms, forms = {}, {}
    for what, call in calls.items():
        before = ctx.pair_paths()
        ctx.timing_enable(True)
        call()
        kernel_ms[what] = {"index_build": round(ctx.timing_read(ga.KERNEL_PAIRS_INDEX)["ms"], 4),
                           "pairs_kernel": round(ctx.timing_read(ga.KERNEL_PAIRS)["ms"], 4)}
        ctx.timing_enable(False)
        after = ctx.pair_paths()
        forms[what] = {key: after[key] - before[key] for key in after if after[key] != before[key]}
    return {"input": name, "rows": n, "sketch_size": s, "min_ani": float(MIN_ANI), "steps": steps,
            "library": os.path.relpath(ga.LIB_PATH, ROOT), "new_rows": {w: n - m for w, m in n_old.items()},
            "pairs": pairs, "ms": {w: stats(v) for w, v in times.items()}, "kernel_ms": kernel_ms, "k2_form": forms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--full-only", action="store_true", help="time the all-pairs call alone (any library build)")
    ap.add_argument("--tag", default="", help="suffix of the JSON file names under --out")
    ap.add_argument("--out", help="directory for one JSON file per input")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "border_flow.py needs a GPU"
    for name in a.inputs.split(","):
        with ga.Context(k=K, sketch_size=INPUTS[name][1], seed=0, device=0) as ctx:
            line = json.dumps(measure(ctx, name, a.steps, a.full_only))
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name + (("_" + a.tag) if a.tag else "") + ".json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
