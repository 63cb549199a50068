"""K1's bottom-s selection at the sketch sizes where its geometry switches,
and the tau search on its own.

sketch_geom (api.cpp) derives from s the candidate limit, the finalize's LDS
sort size and the oversampling of the first tau; the finalize kernel's block
size, bucket bits and dynamic LDS follow from the sort size
(launch_sketch_finalize, sketch.hip).  The sizes here are 1, kMaxSketch and
both sides of every switch; the genomes hold k-mer counts around s and around
the count at which the first tau leaves 2^64 - 1.

GALAHGPU_TAU_OVER (read once per process, so in a child process) sends
ordinary genomes through the whole search: too few candidates, a list that
outgrows the sort, a set that does, bisection.

Everything is compared with the CPU oracle bit for bit, lengths included.
The sketching tests need an MI355X.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import galah_amd as ga
import oracle
from test_k1_stretch import crossing_genomes, rnd

K = 21
SIZES = (1, 2, 32, 33, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12000)
MAX_SKETCH = 12000  # kMaxSketch of gg_internal.hpp
SORT_CAP = 16384    # kSortCap of gg_internal.hpp


def geom(s):
    """sketch_geom of api.cpp: (limit, sort_pow2, over)."""
    limit = min(SORT_CAP, max(2 * s, 64))
    sort_pow2 = 1
    while sort_pow2 < limit:
        sort_pow2 <<= 1
    return limit, sort_pow2, min(2.0, 0.8 * limit / s)


def first_tau_is_max(nk, s):
    """first_tau of gg_internal.hpp leaves tau at 2^64 - 1 unless the expected
    candidates over * s are fewer than the genome's k-mers."""
    return not (nk != 0 and geom(s)[2] * s < nk)


def finalize_threads(s):
    """launch_sketch_finalize of sketch.hip."""
    return 1024 if geom(s)[1] >= 4096 else 256


def finalize_lds(s):
    """launch_sketch_finalize of sketch.hip: the values, then 2^nb_log2 u32 bucket counters."""
    sort_pow2 = geom(s)[1]
    nb_log2 = 6
    while nb_log2 < 12 and (1 << (nb_log2 + 2)) < sort_pow2:
        nb_log2 += 1
    return 8 * sort_pow2 + (4 << nb_log2), nb_log2


def test_sizes_straddle_the_switches():
    """The facts the cases below rely on."""
    assert max(SIZES) == MAX_SKETCH
    # the floor of 64 candidates: 2 s reaches it at s = 32
    assert [geom(s)[:2] for s in (1, 2, 32, 33)] == [(64, 64), (64, 64), (64, 64), (66, 128)]
    # under the floor the oversampling grows beyond 1.6 and is capped at 2
    assert geom(1)[2] == geom(2)[2] == 2.0 and abs(geom(32)[2] - 1.6) < 1e-12 and abs(geom(33)[2] - 1.6) < 1e-12
    # the 1024-thread finalize from a sort of 4096 entries
    assert (geom(1024)[1], geom(1025)[1]) == (2048, 4096)
    assert (finalize_threads(1024), finalize_threads(1025)) == (256, 1024)
    # dynamic LDS above 64 KB from a sort of 8192 entries
    assert (geom(2048)[1], geom(2049)[1]) == (4096, 8192)
    assert finalize_lds(2048)[0] <= 65536 < finalize_lds(2049)[0]
    # the largest sort, and the largest bucket count
    assert (geom(4096)[1], geom(4097)[1]) == (8192, SORT_CAP)
    assert [finalize_lds(s)[1] for s in (1, 33, 1024, 1025, 2049, 4097)] == [6, 6, 9, 10, 11, 12]
    # the cap on the limit: 2 s passes it at s = 8193, and the oversampling falls below 1.6
    assert geom(8192) == (SORT_CAP, SORT_CAP, 1.6)
    assert geom(8193)[:2] == (SORT_CAP, SORT_CAP) and geom(8193)[2] < 1.6
    assert 1.09 < geom(MAX_SKETCH)[2] < 1.1
    for s in SIZES:
        limit, sort_pow2, over = geom(s)
        assert s < limit <= sort_pow2
        n = int(over * s)
        assert first_tau_is_max(n, s) and not first_tau_is_max(n + 1, s)


def genome_of(rng, n):
    """One record of n k-mers (none: a record too short for one)."""
    return (rnd(rng, n + K - 1),)


@functools.lru_cache(maxsize=None)
def size_genomes(s):
    rng = np.random.default_rng(700 + s)
    n_over = int(geom(s)[2] * s)
    r = rnd(rng, 4 * s + K - 1)
    half = rnd(rng, n_over // 2 + K - 1)
    return (
        genome_of(rng, s - 1),
        genome_of(rng, s),
        genome_of(rng, s + 1),
        genome_of(rng, n_over),          # the first tau is still 2^64 - 1
        genome_of(rng, n_over + 1),      # the first count at which it is not
        genome_of(rng, 8 * s + 1000),
        (r, r),                          # every candidate twice: too few distinct, then the search
        (half, half),                    # every candidate twice at tau = 2^64 - 1: ranked among the first copies
        (),
    )


@pytest.mark.gpu
@pytest.mark.parametrize("s", SIZES)
def test_sketch_size(s):
    """K-mer counts around s and around floor(over s), a long genome, genomes
    whose every k-mer occurs twice (the finalize counts and ranks the first
    copies, in 16-bit halves of its bucket counters, at this sort size) and an
    empty one, in one call; alone as well at the smallest sizes and at
    kMaxSketch."""
    genomes = size_genomes(s)
    assert len(genomes[6][0]) - K + 1 == 4 * s
    assert first_tau_is_max(2 * (len(genomes[7][0]) - K + 1), s)
    expected = [oracle.sketch_records(list(g), k=K, s=s, seed=0) for g in genomes]
    for n, e in zip((s - 1, s, s), expected[:3]):  # (random 21-mers: all distinct)
        assert len(e) == n
    calls = [list(range(len(genomes)))]
    if s <= 33 or s == MAX_SKETCH:
        calls += [[g] for g in range(len(genomes))]
    with ga.Context(k=K, sketch_size=s, seed=0) as ctx:
        for call in calls:
            sk, lens = ctx.sketch(ga.pack_records([genomes[g] for g in call], k=K))
            assert sk.shape == (len(call), s)
            for row, g in enumerate(call):
                exp = expected[g]
                assert lens[row] == len(exp), (s, call, g, int(lens[row]), len(exp))
                assert (sk[row][:lens[row]] == exp).all(), (s, call, g)


# ----------------------------------------------------- forced tau search ----
def forced_inputs():
    """The inputs of the forced search, one Context.sketch call each."""
    rng = np.random.default_rng(800)
    r = rnd(rng, 30000)
    return [list(crossing_genomes(K)), [(rnd(rng, 100000),)], [(r, r)]]


_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import galah_amd as ga
from test_k1_sketch_sizes import K, forced_inputs
out = {}
with ga.Context(k=K, sketch_size=1000, seed=0) as ctx:
    for i, genomes in enumerate(forced_inputs()):
        sk, lens = ctx.sketch(ga.pack_records(genomes, k=K))
        out["sk%d" % i], out["lens%d" % i] = sk, lens
    fb = ctx.fallbacks()
out["fb_names"] = np.array(sorted(fb))
out["fb_counts"] = np.array([fb[n] for n in sorted(fb)], np.uint64)
np.savez(sys.argv[3], **out)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("over", ["0.01", "1.9"])
def test_forced_tau_search(over):
    """GALAHGPU_TAU_OVER=0.01: the first tau expects 10 candidates where 1000
    are needed, so every genome with more k-mers than that goes through the
    search: tau times four while too few, a list longer than the sort (the
    same tau again in set mode), a set larger than the sort, bisection.  1.9:
    1900 expected of the 2000 the limit allows.  api.cpp says any value gives
    the same sketches."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GALAHGPU_TAU_OVER=over)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "forced.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(here), here, path], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(path) as z:
            got = {n: z[n].copy() for n in z.files}
    fb = dict(zip((str(n) for n in got["fb_names"]), (int(c) for c in got["fb_counts"])))
    for i, genomes in enumerate(forced_inputs()):
        sk, lens = got["sk%d" % i], got["lens%d" % i]
        assert sk.shape == (len(genomes), 1000) and lens.shape == (len(genomes),)
        for g, recs in enumerate(genomes):
            exp = oracle.sketch_records(list(recs), k=K, s=1000, seed=0)
            assert lens[g] == len(exp), (over, i, g, int(lens[g]), len(exp), fb)
            assert (sk[g][:lens[g]] == exp).all(), (over, i, g, fb)
    if over == "0.01":  # the chain ran
        assert fb["sketch_retry"] > 0 and fb["sketch_set"] > 0, fb
