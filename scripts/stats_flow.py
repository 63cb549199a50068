#!/usr/bin/env python3
"""Wall time of galah's front end (assembly statistics + sketches) on the
file set of bench.py --full's files leg: N synthetic 3 Mbp genomes as gzip
FASTA (80 columns, zlib level 6, one member).

  fused      ctx.sketch_files_stats(paths)            one read of each file
  sketch     ctx.sketch_files(paths)                  the sketches alone
  two_read   ctx.sketch_files(paths) then ga.genome_stats(paths, threads)
             the flow galah has today: every file read and decoded twice

Each is the median of --steps calls after one warm-up call, in one process,
interleaved call by call so that they see the same machine state.  The
library is the one GALAHGPU_LIB names (a build of another commit has no
fused call: it is then skipped), so `sketch` can be taken at two commits
with the same files (--keep DIR writes the files once and reuses them).
Prints one JSON line.

    python scripts/stats_flow.py --genomes 1000 --steps 5 [--keep DIR] [--out FILE]
"""
import argparse
import concurrent.futures as cf
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import galah_amd as ga  # noqa: E402


def write_files(d, n, glen, threads):
    """bench.py's files leg genomes (synth_device, clusters of 10) as gzip FASTA."""
    with ga.Context(k=21, sketch_size=1000, seed=0, device=0) as ctx:
        d_words = torch.empty(n * glen // 16, dtype=torch.int32, device="cuda:0")
        ctx.synth_device(n, glen, 10, 0.07, 3, d_words)  # (bench.py's defaults: --cluster, --max-sub, --seed)
        torch.cuda.synchronize(0)
        words = d_words.cpu().numpy().view(np.uint32)
        del d_words
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    shifts = (np.uint32(30) - 2 * np.arange(16, dtype=np.uint32))[None, :]
    nl = np.full((glen // 80, 1), ord("\n"), np.uint8)

    def write(g):
        w = words[g * glen // 16:(g + 1) * glen // 16]
        seq = acgt[((w[:, None] >> shifts) & np.uint32(3)).reshape(-1)]
        body = np.concatenate([seq[: glen // 80 * 80].reshape(-1, 80), nl], axis=1).tobytes()
        text = b">genome_%d synthetic C2\n" % g + body + (bytes(seq[glen // 80 * 80:]) + b"\n" if glen % 80 else b"")
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        p = os.path.join(d, "g%05d.fna.gz" % g)
        with open(p, "wb") as fh:
            fh.write(c.compress(text) + c.flush())
        return p

    with cf.ThreadPoolExecutor(threads) as ex:
        return list(ex.map(write, range(n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--genome-len", type=int, default=3000000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads (ingest and genome_stats)")
    ap.add_argument("--keep", help="directory for the files (written when empty, reused otherwise, not removed)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    d = a.keep or tempfile.mkdtemp(prefix="gg_stats_flow_")
    os.makedirs(d, exist_ok=True)
    try:
        paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".fna.gz"))
        if len(paths) != a.genomes:
            t0 = time.perf_counter()
            paths = write_files(d, a.genomes, a.genome_len, a.threads)
            print("[stats_flow] wrote %d files in %.1f s" % (len(paths), time.perf_counter() - t0), file=sys.stderr,
                  flush=True)
        fused_ok = hasattr(ga.lib(), "gg_sketch_files_stats")
        times = {"sketch": [], "two_read": []}
        if fused_ok:
            times["fused"] = []
        with ga.Context(k=21, sketch_size=1000, seed=0, device=0, host_threads=a.threads) as ctx:
            sk0, l0, _ = ctx.sketch_files(paths)  # warm-up (device buffers sized for the batches)
            if fused_ok:
                sk1, l1, st1 = ctx.sketch_files_stats(paths)
                assert (sk1 == sk0).all() and (l1 == l0).all()
                host = ga.genome_stats(paths, threads=a.threads)
                assert st1 == host and all(x.total_bases == y.total_bases for x, y in zip(st1, host))
            for _ in range(a.steps):
                if fused_ok:
                    t = time.perf_counter()
                    ctx.sketch_files_stats(paths)
                    times["fused"].append(time.perf_counter() - t)
                t = time.perf_counter()
                ctx.sketch_files(paths)
                times["sketch"].append(time.perf_counter() - t)
                t = time.perf_counter()
                ctx.sketch_files(paths)
                if fused_ok:
                    ga.genome_stats(paths, threads=a.threads)
                times["two_read"].append(time.perf_counter() - t)
            kernels = {}
            if fused_ok:  # the parse passes' HIP-event time, with and without the statistics
                for name, call in (("sketch", ctx.sketch_files), ("fused", ctx.sketch_files_stats)):
                    ctx.timing_enable(True)
                    call(paths)
                    kernels[name] = {"parse": ctx.timing_read(ga.KERNEL_PARSE), "k1": ctx.timing_read(ga.KERNEL_SKETCH)}
                ctx.timing_enable(False)
            info = ctx.info_line()
        if not fused_ok:
            del times["two_read"]  # (no genome_stats in this library: it would time sketch_files alone)
        res = {"workload": "%d x %d bp gzip FASTA (80 columns, zlib level 6), k=21, s=1000" % (a.genomes, a.genome_len),
               "lib": os.path.relpath(ga.LIB_PATH, ROOT), "host_threads": a.threads, "steps": a.steps,
               "median_s": {k: round(float(np.median(v)), 4) for k, v in times.items()},
               "all_s": {k: [round(x, 4) for x in v] for k, v in times.items()},
               "kernel_ms": kernels, "info_line": info}
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        if not a.keep:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
