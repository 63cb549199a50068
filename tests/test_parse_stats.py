"""The statistics passes' per-thread masks (galah_amd/csrc/parse_core.hpp:
stat_roles and record_counts, used by parse.hip passes 4 and 5) on the host,
against a byte-by-byte restatement over 400k random 32-byte chunks
(tests/cpp/test_parse_stats.cpp).  The kernels themselves are checked end to
end in test_genome_stats_gpu.py (GPU).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_stat_masks_equal_bytewise_rules():
    src = os.path.join(ROOT, "tests", "cpp", "test_parse_stats.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_parse_stats")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 400000")
