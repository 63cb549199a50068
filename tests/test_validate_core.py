"""The shared rules of cluster validation (galah_amd/csrc/validate_core.hpp:
finch's merge and the rank formula the named-pair kernel computes it by, the
two f32 comparisons, the lowered threshold that makes the all-pairs path a
superset of the representative rule, the member list) driven on the host by
tests/cpp/test_validate_core.cpp.  The kernel itself is checked in
test_validate_gpu.py (GPU).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_validation_rules():
    src = os.path.join(ROOT, "tests", "cpp", "test_validate_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_validate_core")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 100000
