"""The tail of K1's hash and its tau prefilter (galah_amd/csrc/sketch_core.hpp)
driven on the host by tests/cpp/test_sketch_core.cpp: exact_hash against
murmur3's finaliser written out on its own; the high word of the hash within
one of the high word of (f1 + f2) * C2, all three differences seen; and no
k-mer with hash <= tau that the prefilter drops, over 4 * 10^6 random
(f1, f2, tau) and over cases built by inverting C2 onto tau's high word, its
neighbours and the low-word carries, for hi(tau) from 0 to 2^32 - 1.  The
kernel's use of it is checked in test_k1_prefilter_gpu.py (GPU).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_hash_tail_and_prefilter_have_no_false_negative():
    src = os.path.join(ROOT, "tests", "cpp", "test_sketch_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_sketch_core")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert len(ok) == 1 and int(ok[0].split()[1]) >= 6000000, r.stdout
    assert "FAIL" not in r.stdout, r.stdout
    assert any(ln.startswith("info hi(tau)=2^21") for ln in r.stdout.splitlines()), r.stdout
