"""Times the dense ANI matrix (gg_ani_matrix_device) against the
only other way to every pair's counts and ANI on the device: the gate kernel
at min_ani = 0 (gg_pairs_device) followed by gg_ani_f32_device.

Inputs: m resident rows at sketch size s, in clusters of a given size.  A
cluster's rows are model sketches: a base of s random 64-bit hashes, each
member replacing a fraction of them by hashes of its own (the rows of
different clusters share nothing).  Both paths read the same rows.  Per input:
a warm-up call, then the median and the spread of `--calls` timed calls
(wall clock around a synchronising call), for the matrix with all three
outputs, the matrix with `common` alone (no ANI pass) and the baseline; the
two paths' results are compared on a sample of pairs.  One JSON line per
input; --out writes them to a file as well.

    python scripts/ani_matrix_bench.py --m 10000 --clusters 10 1000 5000

--groups times the grouped form (gg_ani_matrix_groups_device)
instead: every cluster is a group, and the same cells are produced by the
grouped call, by the one matrix over all rows (m <= 32,768) and by the named-pair kernel over every group's
pairs (a <= b) followed by gg_ani_f32_device; 100,000 sampled cells of each
are compared with the grouped result.

    python scripts/ani_matrix_bench.py --groups --m 100000 --clusters 10
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


def model_rows(m, s, cluster, replace, seed):
    rng = np.random.default_rng(seed)
    sk = np.empty((m, s), np.uint64)
    n_rep = max(1, int(s * replace))
    for c0 in range(0, m, cluster):
        base = rng.integers(1, 2 ** 63, s, dtype=np.uint64)
        for g in range(c0, min(c0 + cluster, m)):
            row = base.copy()
            row[rng.choice(s, n_rep, replace=False)] = rng.integers(1, 2 ** 63, n_rep, dtype=np.uint64)
            sk[g] = np.sort(row)
    assert all(len(np.unique(r)) == s for r in sk[:: max(1, m // 50)])
    return sk, np.full(m, s, np.uint32)


def timed(fn, calls):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": calls}


def groups_input(ctx, ga, m, s, cluster, replace, calls, one_group=False, alone=False):
    """One input of the groups mode: m rows in clusters (= groups) of `cluster`;
    one_group: the same rows as a single group of m (against the one matrix);
    alone: the grouped call only (under a kernel trace)."""
    import torch
    sk, lens = model_rows(m, s, cluster, replace, seed=cluster)
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    offsets = np.minimum(np.arange(0, m + cluster, cluster), m).astype(np.uint32)
    if one_group:
        offsets = np.array([0, m], np.uint32)
    sizes = np.diff(offsets).astype(np.int64)
    cell_off = ga.ani_matrix_group_cells(offsets).astype(np.int64)
    cells = int(cell_off[-1])
    d_members = torch.arange(m, dtype=torch.int32, device="cuda")
    d_common = torch.zeros(cells, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(cells, dtype=torch.int32, device="cuda")
    d_ani = torch.zeros(cells, dtype=torch.float32, device="cuda")
    summary = {}

    def grouped():
        summary.update(ctx.ani_matrix_groups_device(d_sk, d_lens, m, d_members, offsets, d_common, d_total, d_ani))

    res = {"input": "m=%d s=%d %s of %d" % (m, s, "one group, clusters" if one_group else "groups", cluster), "n_groups": len(sizes), "cells": cells}
    res["groups"] = timed(grouped, calls)
    res["summary"] = dict(summary)
    if alone:
        return res

    # 100,000 sampled cells: (group, a, b) -> the cell, its rows
    rng = np.random.default_rng(1)
    g = rng.integers(0, len(sizes), 100000)
    a, b = (rng.random(100000) * sizes[g]).astype(np.int64), (rng.random(100000) * sizes[g]).astype(np.int64)
    cell = torch.from_numpy(cell_off[g] + a * sizes[g] + b).cuda()
    ra, rb = torch.from_numpy(offsets[g].astype(np.int64) + a).cuda(), torch.from_numpy(offsets[g].astype(np.int64) + b).cuda()
    got = (d_common[cell], d_total[cell], d_ani[cell].view(torch.int32))

    if m <= 32768:
        m_common = torch.zeros((m, m), dtype=torch.int32, device="cuda")
        m_total = torch.zeros((m, m), dtype=torch.int32, device="cuda")
        m_ani = torch.zeros((m, m), dtype=torch.float32, device="cuda")
        res["matrix_all_rows"] = timed(lambda: ctx.ani_matrix_device(d_sk, d_lens, m, None, m, m_common, m_total, m_ani),
                                       calls)
        assert torch.equal(m_common[ra, rb], got[0]) and torch.equal(m_total[ra, rb], got[1])
        assert torch.equal(m_ani[ra, rb].view(torch.int32), got[2])
        res["matrix_sample_equal"] = True
        del m_common, m_total, m_ani

    if one_group:
        return res
    # the named pairs (a <= b) of every group; pair_at[g] the first pair of group g, row a's pairs in b order
    tri = sizes * (sizes + 1) // 2
    pair_at = np.concatenate([[0], np.cumsum(tri)])
    n_pairs = int(pair_at[-1])
    d_pairs = torch.zeros((n_pairs, 4), dtype=torch.int32, device="cuda")
    at = 0
    for size in np.unique(sizes):  # (the groups of one size at once)
        gs = torch.from_numpy(np.flatnonzero(sizes == size)).cuda()
        iu = torch.triu_indices(int(size), int(size), device="cuda")
        first = torch.from_numpy(offsets[:-1].astype(np.int64)).cuda()[gs]
        base = torch.from_numpy(pair_at[:-1]).cuda()[gs]
        where = (base[:, None] + torch.arange(iu.shape[1], device="cuda")[None, :]).reshape(-1)
        d_pairs[where, 0] = (first[:, None] + iu[0][None, :]).reshape(-1).int()
        d_pairs[where, 1] = (first[:, None] + iu[1][None, :]).reshape(-1).int()
        at += len(gs) * iu.shape[1]
    assert at == n_pairs
    d_pani = torch.zeros(n_pairs, dtype=torch.float32, device="cuda")

    def named():
        ctx.ani_pairs_device(d_sk, d_lens, m, d_pairs, n_pairs)
        torch.cuda.synchronize()
        ctx.ani_f32_device(d_pairs, n_pairs, d_pani)

    res["named_pairs"] = n_pairs
    res["ani_pairs_then_ani_f32"] = timed(named, calls)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    which = torch.from_numpy(pair_at[g] + lo * sizes[g] - lo * (lo - 1) // 2 + (hi - lo)).cuda()
    p = d_pairs[which]
    assert torch.equal(p[:, 2], got[0]) and torch.equal(p[:, 3], got[1])
    assert torch.equal(d_pani[which].view(torch.int32), got[2])
    res["named_sample_equal"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--sketch", type=int, default=1000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[10, 1000, 5000], help="cluster sizes, one input each")
    ap.add_argument("--replace", type=float, default=0.05, help="fraction of a member's hashes that are its own")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--groups", action="store_true", help="the grouped form: every cluster a group")
    ap.add_argument("--one-group", action="store_true", help="with --groups: all rows as one group")
    ap.add_argument("--alone", action="store_true", help="with --groups: the grouped call only, nothing to compare with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    os.environ["GALAHGPU_PAIRS_KERNEL"] = "gate"  # the baseline is the gate kernel, whatever "auto" would take
    import galah_amd as ga

    m, s = a.m, a.sketch
    lines = []
    with ga.Context(k=21, sketch_size=s, seed=0, device=0) as ctx:
        for cluster in a.clusters:
            if a.groups:
                res = groups_input(ctx, ga, m, s, cluster, a.replace, a.calls, a.one_group, a.alone)
                print(json.dumps(res), flush=True)
                lines.append(res)
                continue
            sk, lens = model_rows(m, s, cluster, a.replace, seed=cluster)
            d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
            d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
            d_common = torch.zeros((m, m), dtype=torch.int32, device="cuda")
            d_total = torch.zeros((m, m), dtype=torch.int32, device="cuda")
            d_ani = torch.zeros((m, m), dtype=torch.float32, device="cuda")
            summary = {}

            def matrix_all():
                summary.update(ctx.ani_matrix_device(d_sk, d_lens, m, None, m, d_common, d_total, d_ani))

            def matrix_common():
                ctx.ani_matrix_device(d_sk, d_lens, m, None, m, d_common, None, None)

            res = {"input": "m=%d s=%d clusters of %d" % (m, s, cluster), "matrix_all": timed(matrix_all, a.calls),
                   "matrix_common_only": timed(matrix_common, a.calls), "summary": dict(summary)}
            if not a.no_baseline:
                n_pairs = m * (m - 1) // 2
                d_pairs = torch.zeros((n_pairs, 4), dtype=torch.int32, device="cuda")
                d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
                d_pani = torch.zeros(n_pairs, dtype=torch.float32, device="cuda")

                def baseline():
                    d_count.zero_()
                    ctx.pairs_device(d_sk, d_lens, m, 0, ga.pair_tiles(m), 0.0, d_pairs, n_pairs, d_count)
                    torch.cuda.synchronize()
                    ctx.ani_f32_device(d_pairs, int(d_count.item()), d_pani)

                res["pairs_gate_then_ani_f32"] = timed(baseline, a.calls)
                assert int(d_count.item()) == n_pairs
                # the same answers: a sample of the pair list against the matrix
                idx = torch.randint(0, n_pairs, (100000,), device="cuda")
                p = d_pairs[idx].long()
                i, j = p[:, 0] & 0xFFFFFFFF, p[:, 1] & 0xFFFFFFFF
                assert torch.equal(d_common[i, j].long(), p[:, 2]) and torch.equal(d_total[i, j].long(), p[:, 3])
                assert torch.equal(d_ani[i, j].view(torch.int32), d_pani[idx].view(torch.int32))
                res["sample_equal"] = True
                res["speedup_all"] = round(res["pairs_gate_then_ani_f32"]["median_ms"] / res["matrix_all"]["median_ms"], 2)
                del d_pairs, d_pani
            print(json.dumps(res), flush=True)
            lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
