"""The device precluster step's shared rules (galah_amd/csrc/precluster_core.hpp:
the hook step, the jump step and the sort keys that the kernels of
precluster.hip use) driven on the host by tests/cpp/test_precluster_core.cpp:
the hook step on 8 threads over every case of preclusters_cases.py and under
stale-read schedules against a plain union-find, the jump rounds within their
bound, the keys' round trip, order and width.  The kernels themselves are
checked in test_preclusters_gpu.py (GPU).  CPU only."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import preclusters_cases as pcs
from conftest import ROOT


def test_hook_jump_and_keys():
    src = os.path.join(ROOT, "tests", "cpp", "test_precluster_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_precluster_core")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-pthread", "-o", exe, src])
    cases = pcs.all_cases()
    with tempfile.TemporaryDirectory() as d:
        files = []
        for name, (n, pairs) in cases.items():
            ij = np.stack([pairs["i"], pairs["j"]], axis=1).astype("<u4")
            path = os.path.join(d, name + ".bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<IQ", n, len(ij)))
                f.write(ij.tobytes())
            files.append(path)
        r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok %d" % len(cases)
