#!/usr/bin/env python3
"""Wall time of the precluster step on the host and on the
device, same input, same process:

  host      gg_partition_preclusters then gg_precluster_pairs (precluster.cpp),
            one thread: the baseline (host_partition: the first call alone)
  device    gg_preclusters: upload of the pairs (pageable memory), the
            kernels, members / offsets / local pairs / pair_offsets back
  resident  gg_preclusters_device: pairs and outputs in device memory, ended
            by a stream synchronise

The C entry points are called over arrays made once, so no wrapper's copy of
the pair list is in any figure.

Inputs, those of scripts/cluster_flow.py: the 351 golden
pairs; synthetic cluster graphs (genomes in clusters, a pair inside a cluster
kept with the probability that gives the wanted pair count, the genome order
shuffled); the paths (i, i + 1) of 20,000 and 1,000,000 genomes in order,
which the hook launch may leave as one chain.  After one warm-up call of each
form, the three are timed call by call in turn; the median, the minimum and
the maximum of --steps calls are reported, with the HIP-event time of the
step's kernels and the number of jump launches (from a further call).  The
results are compared on every input (local pairs after a sort on
(precluster, i, j, src)).  Prints one JSON line per input; --out DIR also
writes them to DIR/NAME.json.

    python scripts/precluster_flow.py --steps 7 [--out profiles/precluster_flow]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import galah_amd as ga  # noqa: E402
from cluster_flow import PATHS, SYNTH, make_input  # noqa: E402


class Calls:
    """The three forms as their C entry points, over arrays made once: what
    is timed is the library, not the Python wrappers' copies."""

    def __init__(self, ctx, n, pairs):
        self.L, self.c, self.n, self.m = ga.lib(), ctx._c, n, len(pairs)
        self.pairs = np.ascontiguousarray(pairs)
        self.members = np.zeros(max(n, 1), np.uint32)
        self.offsets = np.zeros(n + 1, np.uint32)
        self.local = np.zeros(max(self.m, 1), ga.LOCAL_PAIR_DTYPE)
        self.poff = np.zeros(n + 1, np.uint64)
        self.ns = ctypes.c_uint32()
        self.p = [x.ctypes.data_as(ctypes.c_void_p) for x in (self.pairs, self.members, self.offsets, self.local,
                                                              self.poff)]

    def _ok(self, st):
        if st != 0:
            raise RuntimeError("status %d: %s" % (st, self.L.gg_thread_last_error().decode()))

    def host_partition(self):
        self._ok(self.L.gg_partition_preclusters(self.n, self.p[0], self.m, self.p[1], self.p[2],
                                                 ctypes.byref(self.ns)))

    def host_pairs(self):
        self._ok(self.L.gg_precluster_pairs(self.n, self.p[0], self.m, self.p[1], self.p[2], self.ns.value,
                                            self.p[3], self.p[4]))

    def device(self):
        self._ok(self.L.gg_preclusters(self.c, self.n, self.p[0], self.m, self.p[1], self.p[2],
                                       ctypes.byref(self.ns), self.p[3], self.p[4]))

    def resident(self, ptrs):
        # (the call ends with a stream synchronise of its own)
        self._ok(self.L.gg_preclusters_device(self.c, self.n, ptrs[0], self.m, ptrs[1], ptrs[2],
                                              ctypes.byref(self.ns), ptrs[3], ptrs[4], None))

    def result(self):
        ns = self.ns.value
        return (self.members[:self.n].copy(), self.offsets[:ns + 1].copy(), self.local[:self.m].copy(),
                self.poff[:ns + 1].copy())


def same(a, b):
    def key(local):
        return local[np.lexsort((local["src"], local["j"], local["i"], local["precluster"]))].tobytes()
    return (a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[3].tolist() == b[3].tolist()
            and key(a[2]) == key(b[2]))


def measure(ctx, name, n, pairs, steps):
    device = "cuda:%d" % ctx.device
    m = len(pairs)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).copy()).to(device)
    d_members = torch.zeros(n, dtype=torch.int32, device=device)
    d_offsets = torch.zeros(n + 1, dtype=torch.int32, device=device)
    d_local = torch.zeros(4 * m, dtype=torch.int32, device=device)
    d_poff = torch.zeros(n + 1, dtype=torch.int64, device=device)
    ptrs = [t.data_ptr() for t in (d_pairs, d_members, d_offsets, d_local, d_poff)]
    torch.cuda.synchronize()

    call = Calls(ctx, n, pairs)
    # warm-up: scratch sized, code objects loaded; and the three forms agree
    call.host_partition()
    call.host_pairs()
    host = call.result()
    call.device()
    dev = call.result()
    call.resident(ptrs)
    ns = call.ns.value
    res = (d_members.cpu().numpy().view(np.uint32), d_offsets.cpu().numpy().view(np.uint32)[:ns + 1],
           d_local.cpu().numpy().view(ga.LOCAL_PAIR_DTYPE), d_poff.cpu().numpy().view(np.uint64)[:ns + 1])
    assert same(dev, host) and same(res, host), name
    times = {"host": [], "host_partition": [], "device": [], "resident": []}
    for _ in range(steps):
        t = time.perf_counter()
        call.host_partition()
        t1 = time.perf_counter()
        call.host_pairs()
        t2 = time.perf_counter()
        times["host"].append(t2 - t)
        times["host_partition"].append(t1 - t)
        t = time.perf_counter()
        call.device()
        times["device"].append(time.perf_counter() - t)
        t = time.perf_counter()
        call.resident(ptrs)
        times["resident"].append(time.perf_counter() - t)
    ctx.timing_enable(True)
    call.resident(ptrs)
    k = ctx.timing_read(ga.KERNEL_PRECLUSTER)
    ctx.timing_enable(False)
    jumps = int(ctx.info_line().split("precluster jump launches ")[1].split(";")[0])
    return {"input": name, "genomes": n, "pairs": int(m), "preclusters": int(len(host[1]) - 1), "steps": steps,
            "jump_launches": jumps, "kernel_launches": int(k["launches"]), "kernel_ms": round(k["ms"], 4),
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
            n, pairs, _ = make_input(name)
            line = json.dumps(measure(ctx, name, n, pairs, a.steps))
            print(line, flush=True)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, name + ".json"), "w") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
