#!/usr/bin/env python3
"""Wall time of asking about genomes that are not to be added:
the query against what the library could do before it, same process, same
rows, the two routes alternating call by call.

  (a) gg_query_rows_device + gg_ani_f32_device: a table of the queries, the
      resident rows streamed against it once;
  (b) gg_pairs_border_device over the same matrix with the queries in spare
      rows after row N (written there before the clock), n_old = N, on the
      default pairs path, + gg_ani_f32_device; its hits are the border pairs
      with i < N (it also evaluates the query x query pairs).

Inputs: the MinHash model of scripts/border_flow.py (clusters of 10, shuffled
rows, s = 1000) resident in HBM at N = 10,000 and 100,000; Q = 1, 100 and 1,000
queries, half of them further members of the rows' clusters and half unrelated;
and one query against a single cluster of 5,000.  Each call ends in a device
synchronise and is timed with the host clock after one warm-up; median
[min - max] of --steps calls.  The two routes' hits are asserted equal on
every input.  Prints one JSON line per input; --out DIR also writes
DIR/NAME.json.

    python scripts/query_flow.py --steps 7 [--out profiles/query_flow] [--only n10k]
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
from border_flow import sorted_quads, stats, synth_sketches  # noqa: E402

MIN_ANI = np.float32(0.95)
K, S = 21, 1000
LENGTHS = (3e6, 3e6)
QUERIES = (1, 100, 1000)


def clock(f):
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def measure(ctx, name, d_rows, d_queries, steps):
    """d_rows [N, s], d_queries [Q, s] (int64 holding the hashes) -> the case's figures."""
    n, nq = d_rows.shape[0], d_queries.shape[0]
    d_all = torch.cat([d_rows, d_queries]).contiguous()  # route (b)'s matrix: the queries after row N
    d_lens = torch.full((n + nq,), S, dtype=torch.int32, device="cuda")
    cap = 1 << 21
    out = [torch.empty((cap * 4,), dtype=torch.int32, device="cuda") for _ in range(2)]
    ani = [torch.empty((cap,), dtype=torch.float32, device="cuda") for _ in range(2)]
    cnt = [torch.zeros((1,), dtype=torch.int64, device="cuda") for _ in range(2)]
    thr = float(MIN_ANI)

    def query():
        cnt[0].zero_()
        ctx.query_rows_device(d_rows, d_lens, n, d_queries, d_lens[n:], nq, thr, out[0], cap, cnt[0])
        ctx.ani_f32_device(out[0], int(cnt[0].item()), ani[0])

    def border():
        cnt[1].zero_()
        ctx.pairs_border_device(d_all, d_lens, n + nq, n, thr, out[1], cap, cnt[1])
        ctx.ani_f32_device(out[1], int(cnt[1].item()), ani[1])

    t = {"query": [], "border": []}
    for step in range(steps + 1):  # (the first round warms both routes up)
        ta, tb = clock(query), clock(border)
        if step:
            t["query"].append(ta)
            t["border"].append(tb)
    ca, cb = int(cnt[0].item()), int(cnt[1].item())
    assert ca <= cap and cb <= cap, (name, ca, cb)
    qa, qb = sorted_quads(out[0], ca), sorted_quads(out[1], cb)
    qb = qb[qb[:, 0] < n]
    assert qa.shape == qb.shape and (qa == qb).all(), (name, "the two routes' hits differ")
    a, b = stats(t["query"]), stats(t["border"])
    return {"input": name, "rows": n, "queries": nq, "sketch_size": S, "min_ani": thr, "steps": steps, "hits": ca,
            "border_pairs": cb, "query_ms": a, "border_ms": b,
            "faster": "query" if a["max"] < b["min"] else "border" if b["max"] < a["min"] else "overlap"}


def cases(only):
    for name, n in (("n10k", 10000), ("n100k", 100000)):
        if only and only != name:
            continue
        # the rows are shuffled: the last 500 are further members of the first n rows' clusters
        d_sk, _ = synth_sketches(n + 500, S, LENGTHS)
        d_far, _ = synth_sketches(500, S, LENGTHS, seed=99)
        for q in QUERIES:
            near = (q + 1) // 2
            yield "%s_q%d" % (name, q), d_sk[:n], torch.cat([d_sk[n:n + near], d_far[:q - near]]).contiguous()
        del d_sk, d_far
    if not only or only == "one_cluster":
        d_sk, _ = synth_sketches(5001, S, LENGTHS, cluster=5001)
        yield "one_cluster_5000_q1", d_sk[:5000], d_sk[5000:].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--only")
    args = ap.parse_args()
    with ga.Context(k=K, sketch_size=S) as ctx:
        for name, d_rows, d_queries in cases(args.only):
            line = measure(ctx, name, d_rows, d_queries, args.steps)
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, name + ".json"), "w") as f:
                    json.dump(line, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
