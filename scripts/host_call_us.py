"""The binding's cost per call on the CPU: microseconds per call of ani_pairs_host on one pair
of 4-hash rows (through the call frame) and of pair_tiles(3) (a bare ctypes call, the yardstick for the
machine's own spread), 10^5 calls each, five repeats.  No device is needed.

The module file is executed as a plain module over the library named, so that another commit's
galah_amd/__init__.py can be timed against the same library:

    python scripts/host_call_us.py SIDE [path/to/galah_amd/__init__.py [path/to/libgalahgpu.so]]

prints one tab-separated row per call: call, SIDE, the five repeats.  profiles/binding_frame/host_call_us.tsv
holds two sessions of two processes per side, parent and head alternating.
"""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPEATS = 100000, 5


def load(init, lib):
    old = os.environ.get("GALAHGPU_LIB")
    os.environ["GALAHGPU_LIB"] = lib
    try:
        spec = importlib.util.spec_from_file_location("galah_amd_timed", init)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            os.environ.pop("GALAHGPU_LIB")
        else:
            os.environ["GALAHGPU_LIB"] = old
    return mod


def timed(fn):
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        out.append((time.perf_counter() - t0) / CALLS * 1e6)
    return out


def main():
    side = sys.argv[1] if len(sys.argv) > 1 else "head"
    init = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "galah_amd", "__init__.py")
    lib = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "galah_amd", "lib", "libgalahgpu.so")
    ga = load(init, lib)
    rows = np.array([[1, 2, 3, 4], [1, 2, 3, 5]], np.uint64)
    lens = np.array([4, 4], np.uint32)
    pair = [(0, 1)]
    for name, fn in (("ani_pairs_host", lambda: ga.ani_pairs_host(rows, lens, pair)), ("pair_tiles", lambda: ga.pair_tiles(3))):
        fn()
        print("\t".join([name, side] + ["%.3f" % x for x in timed(fn)]), flush=True)


if __name__ == "__main__":
    main()
