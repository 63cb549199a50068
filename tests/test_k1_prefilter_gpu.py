"""K1's tau prefilter (sketch.hip, sketch_core.hpp): the test on the high word
of (f1 + f2) * C2 against hi(tau) + 2.  Everything goes through the public
path (pack_records, Context.sketch) and is compared with the CPU oracle bit
for bit: genomes whose tau is 2^64 - 1 (every k-mer passes), genomes on either
side of the k-mer count at which first_tau stops saturating (1.6 s k-mers: the
threshold's saturated and unsaturated forms), long genomes at s = 1000 and
s = 50, other k, a non-zero seed, a tandem repeat whose tau advance_tau moves
and which ends in a set-mode pass, and all of them in one call, so that lanes
of one wave hold different thresholds.

A k-mer on the prefilter's boundary has probability 2^-32: these inputs guard
the plumbing; that the prefilter drops no k-mer is shown on the host
(test_sketch_core.py).  Needs an MI355X.
"""
import functools

import numpy as np
import pytest

import galah_amd as ga
import oracle

pytestmark = pytest.mark.gpu

# first_tau (gg_internal.hpp) is 2^64 - 1 up to over * s k-mers, over = 1.6 at
# s = 1000 (sketch_geom, api.cpp): 1600 k-mers is the last saturated count
SATURATED = (1, 44, 1500)
AROUND = (1599, 1600, 1601, 1602, 1650)
LONG = (20000, 200000)


def rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def genome(n_kmers, k=21):
    """One random record of n_kmers k-mers."""
    rng = np.random.default_rng(7000 + 37 * n_kmers + k)
    return (rnd(rng, n_kmers + k - 1),)


@functools.lru_cache(maxsize=None)
def tandem():
    """40 copies of 5000 random bases: far fewer distinct hashes than k-mers."""
    return (rnd(np.random.default_rng(13), 5000) * 40,)


@functools.lru_cache(maxsize=None)
def expected(recs, k, s, seed):
    out = oracle.sketch_records(list(recs), k=k, s=s, seed=seed)
    out.setflags(write=False)
    return out


def check(ctx, genomes, k, s, seed):
    """Sketch `genomes` in one call and compare every row with the oracle."""
    sk, lens = ctx.sketch(ga.pack_records(list(genomes), k=k))
    for g, recs in enumerate(genomes):
        exp = expected(recs, k, s, seed)
        assert lens[g] == len(exp), (k, s, seed, g, int(lens[g]), len(exp))
        assert (sk[g][:lens[g]] == exp).all(), (k, s, seed, g)


def test_k21_s1000_each_and_together():
    genomes = [genome(n) for n in SATURATED + AROUND + LONG]
    with ga.Context(k=21, sketch_size=1000) as ctx:
        for g in genomes:
            check(ctx, [g], 21, 1000, 0)
        check(ctx, genomes + [tandem()], 21, 1000, 0)


def test_k21_s50():
    genomes = [genome(n) for n in LONG]
    with ga.Context(k=21, sketch_size=50) as ctx:
        for g in genomes:
            check(ctx, [g], 21, 50, 0)
        check(ctx, genomes, 21, 50, 0)


@pytest.mark.parametrize("k,seed", [(5, 0), (32, 0), (21, 12345)])
def test_other_k_and_seed(k, seed):
    with ga.Context(k=k, sketch_size=1000, seed=seed) as ctx:
        check(ctx, [genome(200000, k)], k, 1000, seed)


def test_tandem_repeat_moves_tau_and_runs_set_mode():
    """The repeat's 1600 expected candidates hold ~40 distinct hashes, so tau
    grows until the list outgrows the sort and the genome is hashed again in
    set mode: moved taus and a set-mode pass through the new threshold."""
    with ga.Context(k=21, sketch_size=1000) as ctx:
        check(ctx, [tandem()], 21, 1000, 0)
        fb = ctx.fallbacks()
        assert fb["sketch_set"] >= 1 and fb["sketch_retry"] > 0, fb
