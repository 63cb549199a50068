#!/usr/bin/env python3
"""Wall time of clustering from sketches: today's composition
of host-array calls against the resident call, same process, same sketches:

  composed         ctx.pairs(sk, lens, min_ani) -> the f32 ANI of every pair on
                   the host -> ctx.cluster_pairs(n, pairs, ani, T) ->
                   ga.partition_preclusters(n, pairs); each phase timed.  The
                   ANI here is gg_ani_f32 once per distinct (common, total)
                   spread over the pairs with numpy (a call per pair from
                   Python would measure Python); inside gg_cluster_files the
                   same values come from pairs_with_ani's host threads.
  resident_upload  the host matrix uploaded once (pageable memory), then
                   ctx.cluster_rows_device, then rep_of back
  resident         ctx.cluster_rows_device over rows already in device memory,
                   rep_of left there; and, from a further call, the HIP-event
                   time of ctx.ani_f32_device over the call's pairs

Inputs: 10,000 sketches of 1,000 hashes made on the device from the MinHash
model of border_flow.py (a member keeps each of its cluster's k-mers with
probability (1 - r)^21, r drawn in [0, 0.07)), in clusters of 10, of 1,000
and of 5,000, rows shuffled; min_ani 0.95, T 0.97.

Each call is timed with the host clock after one warm-up call of each, the
three alternating step by step; the median, minimum and maximum of --steps
calls are reported.  rep_of and the summary are compared between the flows on
every input.  Prints one JSON line per input; --out DIR also writes
DIR/NAME.json.

    python scripts/resident_flow.py --steps 7 [--out profiles/resident_flow]
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

MIN_ANI, T = float(np.float32(0.95)), float(np.float32(0.97))
N, S, K, MAX_SUB, LENGTH = 10000, 1000, 21, 0.07, 3e6
INPUTS = {"clusters_of_10": 10, "clusters_of_1000": 1000, "clusters_of_5000": 5000}


def synth_sketches(n, s, cluster, seed=5, device="cuda"):
    """-> (d_sk [n, s] int64 holding the u64 hashes, ascending; d_lens [n] int32)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    clusters = (n + cluster - 1) // cluster
    bound = 2.0 * s / LENGTH * 2.0 ** 64  # (below 2^63)
    out = torch.empty((clusters * cluster, s), dtype=torch.int64, device=device)
    step = max(1, (1 << 24) // (cluster * 2 * s))  # clusters per chunk

    def draw(*shape):
        return (torch.rand(*shape, generator=g, device=device, dtype=torch.float64) * bound).to(torch.int64)

    for c0 in range(0, clusters, step):
        c1 = min(clusters, c0 + step)
        base = draw(c1 - c0, 1, 2 * s)
        rate = MAX_SUB * torch.rand((c1 - c0, cluster, 1), generator=g, device=device, dtype=torch.float64)
        keep = torch.rand((c1 - c0, cluster, 2 * s), generator=g, device=device, dtype=torch.float64) < (1 - rate) ** K
        member = torch.where(keep, base.expand(-1, cluster, -1), draw(c1 - c0, cluster, 2 * s))
        member = torch.sort(member, dim=2).values[:, :, :s]
        out[c0 * cluster:c1 * cluster] = member.reshape(-1, s)
    assert bool((out[:, 1:] > out[:, :-1]).all()), "a repeated hash in a synthetic sketch"
    rows = torch.randperm(clusters * cluster, generator=g, device=device)[:n]
    return out[rows].contiguous(), torch.full((n,), s, dtype=torch.int32, device=device)


def ani_f32_of(pairs):
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, K) for x in u], np.float32)
    return vals[inv]


def stats(v):
    return {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3), "max": round(max(v) * 1e3, 3)}


def measure(ctx, name, steps):
    d_sk, d_lens = synth_sketches(N, S, INPUTS[name])
    sk = d_sk.cpu().numpy().view(np.uint64)
    lens = d_lens.cpu().numpy().view(np.uint32)
    d_rep = torch.empty((N,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    phases = {"pairs": [], "ani": [], "cluster_pairs": [], "partition": []}

    def composed(record):
        t0 = time.perf_counter()
        pairs = ctx.pairs(sk, lens, MIN_ANI)
        t1 = time.perf_counter()
        ani = ani_f32_of(pairs)
        t2 = time.perf_counter()
        rep = ctx.cluster_pairs(N, pairs, ani, T)
        t3 = time.perf_counter()
        _, offsets = ga.partition_preclusters(N, pairs)
        t4 = time.perf_counter()
        if record:
            for key, dt in zip(phases, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                phases[key].append(dt)
        return rep, len(pairs), len(offsets) - 1, int(offsets[1] - offsets[0])

    def resident_upload():
        u_sk = torch.from_numpy(sk.view(np.int64)).cuda()
        u_lens = torch.from_numpy(lens.view(np.int32)).cuda()
        summary, _, _, _ = ctx.cluster_rows_device(u_sk, u_lens, N, MIN_ANI, T, d_rep)
        return d_rep.cpu().numpy().view(np.uint32), summary

    def resident():
        out = ctx.cluster_rows_device(d_sk, d_lens, N, MIN_ANI, T, d_rep)
        torch.cuda.synchronize()
        return out

    rep, n_pairs, n_sets, largest = composed(False)  # warm-up: scratch sized, code objects loaded
    rep_u, summary = resident_upload()
    resident()
    assert (rep_u == rep).all(), name
    assert (summary["n_pairs"], summary["n_preclusters"], summary["largest_precluster"]) == (n_pairs, n_sets, largest)
    times = {"composed": [], "resident_upload": [], "resident": []}
    for _ in range(steps):
        for key, f in (("composed", lambda: composed(True)), ("resident_upload", resident_upload),
                       ("resident", resident)):
            t = time.perf_counter()
            f()
            times[key].append(time.perf_counter() - t)
    # the ANI kernels alone, over the pairs of the last call (ani_f32_device
    # leaves the context's pair scratch as it is)
    summary, p_pairs, _, _ = resident()
    d_ani = torch.empty((max(n_pairs, 1),), dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ani_ms = []
    for _ in range(steps):
        e0.record()
        ctx.ani_f32_device(p_pairs, n_pairs, d_ani)
        e1.record()
        torch.cuda.synchronize()
        ani_ms.append(e0.elapsed_time(e1) * 1e-3)
    return {"input": name, "genomes": N, "sketch_size": S, "cluster_size": INPUTS[name], "min_ani": MIN_ANI,
            "cluster_ani": T, "pairs": n_pairs, "clusters": int((rep == np.arange(N)).sum()),
            "preclusters": n_sets, "largest_precluster": largest, "ani_rechecked": summary["ani_rechecked"],
            "ani_rechecked_share": summary["ani_rechecked"] / max(n_pairs, 1), "pair_passes": summary["pair_passes"],
            "steps": steps, "ms": {k: stats(v) for k, v in times.items()},
            "composed_phases_ms": {k: stats(v) for k, v in phases.items()}, "ani_f32_device_event_ms": stats(ani_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--out", help="directory for one JSON file per input")
    a = ap.parse_args()
    with ga.Context(k=K, sketch_size=S, seed=0, device=0) as ctx:
        for name in a.inputs.split(","):
            line = json.dumps(measure(ctx, name, a.steps))
            print(line, flush=True)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, name + ".json"), "w") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
