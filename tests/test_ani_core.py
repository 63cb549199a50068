"""The f32 ANI rule the device uses (galah_amd/csrc/ani_core.hpp: the value of
ani_f64 operation for operation, and the margin test that flags the entries
whose f32 another log could round differently) driven on the host by
tests/cpp/test_ani_core.cpp: equality with the library's expression over the
grid total <= 2000, common <= 1000 for k = 2, 5, 21, 32; every entry flagged
or unchanged under a log moved by up to 64 ulp; at most 1e-4 of the grid
flagged; the integer-decided entries never flagged.  The kernel itself is
checked in test_resident_gpu.py (GPU).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_value_margin_and_integer_cases():
    src = os.path.join(ROOT, "tests", "cpp", "test_ani_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_ani_core")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].split()[0] == "ok" and int(lines[0].split()[1]) >= 1499500, r.stdout
    print(r.stdout)
