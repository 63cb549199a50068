"""The clustering step's shared rules (galah_amd/csrc/cluster_core.hpp: the
per-vertex decision and the membership key that gg_cluster_pairs_host and the
kernels of cluster.hip both use) driven on the host by
tests/cpp/test_cluster_core.cpp: the decision over every short sequence of
neighbour states, and the key order against (ANI descending, representative
ascending) on a million random pairs.  The kernels themselves are checked in
test_cluster_gpu.py (GPU).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_decision_rule_and_key_order():
    src = os.path.join(ROOT, "tests", "cpp", "test_cluster_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_cluster_core")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 1000000")
