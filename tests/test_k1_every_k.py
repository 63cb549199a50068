"""K1 (sketch.hip) at every k it is compiled for.  launch_sketch_candidates
instantiates sketch_candidates_kernel<K, SEED0> for K = 1..32, and the
instantiations differ in structure: zero, one or two full 16-byte murmur
blocks, a whole-word tail table (tails of 1..5 bases) or one to four tail
group tables, the mask of a partial last group, the shift branch of window64
and the segment length.  A bottom-s sketch of a random genome looks up only
the table entries of the few k-mers with the smallest hashes; here every
entry of every table is looked up by a k-mer whose hash is compared:

  * single-k-mer records at s >= the record count (tau = 2^64 - 1: the sketch
    is every distinct hash), all 4^k k-mers up to k = 7, and from k = 8 one
    self-canonical k-mer per (4-base group, pattern of the group's bases);
  * records of random length, so the bits below a partial last group vary;
  * k <= 5, where a genome holds fewer distinct k-mers than s.

Everything goes through pack_records and Context.sketch and is compared with
the CPU oracle bit for bit, lengths included (test_oracle_every_k.py pins the
oracle itself at every k).  Needs an MI355X.
"""
import functools
import itertools

import numpy as np
import pytest

import galah_amd as ga
import oracle
from test_host import unpack_run
from test_oracle_every_k import N_CANONICAL, all_kmers, canonical, murmur3_x64_128, revcomp, rnd

pytestmark = pytest.mark.gpu

SEED_KS = (2, 7, 12, 18, 21, 26, 32)  # the seeded variant: one k of each tail shape, and two blocks
CASES = [(k, 0) for k in range(1, 33)] + [(k, 12345) for k in SEED_KS]


def seg_len(k):
    """k1_seg_len(k, 4) of gg_internal.hpp."""
    return min((65 - k) // 4 * 4, 48)


def n_groups(k):
    return (k + 3) // 4


def group_patterns(k, q):
    """Every pattern of the valid bases of group q (bases 4q .. 4q+3 below k)."""
    return [bytes(t) for t in itertools.product(b"ACGT", repeat=min(4, k - 4 * q))]


def check(genomes, k, s, seed, note=""):
    """Sketch `genomes` (lists of records) in one call and compare every row with the oracle."""
    with ga.Context(k=k, sketch_size=s, seed=seed) as ctx:
        sk, lens = ctx.sketch(ga.pack_records(genomes, k=k))
    for g, recs in enumerate(genomes):
        exp = oracle.sketch_records(list(recs), k=k, s=s, seed=seed)
        assert lens[g] == len(exp), (k, s, seed, g, int(lens[g]), len(exp), note)
        assert (sk[g][:lens[g]] == exp).all(), (k, s, seed, g, note)
    return sk, lens


@functools.lru_cache(maxsize=None)
def table_records(k):
    """One-k-mer records that reach every table entry of K1 at this k.
    k <= 7: all 4^k k-mers.  k >= 8: for every group and pattern one k-mer
    that is its own canonical form and carries the pattern in the group:
    u m rc(u) with m <= rc(m) for the first group, rc(u) m u for the last, and
    for a group that holds neither end the pattern in place between an A at
    either end (the reverse complement then begins with T)."""
    if k <= 7:
        return tuple(all_kmers(k))
    rng = np.random.default_rng(400 + k)
    last = n_groups(k) - 1

    def middle(n):
        while True:
            m = rnd(rng, n)
            if m <= revcomp(m):
                return m

    recs = []
    for q in range(last + 1):
        for u in group_patterns(k, q):
            if q == 0:
                r = u + middle(k - 2 * len(u)) + revcomp(u)
            elif q == last:
                r = revcomp(u) + middle(k - 2 * len(u)) + u
            else:
                r = bytearray(rnd(rng, k))
                r[0] = r[-1] = ord("A")
                r[4 * q:4 * q + 4] = u
                r = bytes(r)
            assert len(r) == k
            recs.append(r)
    return tuple(recs)


def covered_pairs(recs, k):
    """The (group, pattern) pairs among the canonical forms of one-k-mer records."""
    seen = set()
    for r in recs:
        c = canonical(r)
        for q in range(n_groups(k)):
            seen.add((q, c[4 * q:4 * q + 4]))
    return seen


@pytest.mark.parametrize("k,seed", CASES)
def test_every_table_entry(k, seed):
    """Every (group, pattern) pair of hash_parts' tables contributes a compared
    hash.  The completeness of the inputs is asserted first, no pair left out;
    up to k = 7 the inputs are all 4^k k-mers instead (a k-mer shorter than 8
    bases cannot carry every pattern in its canonical form: TTTT.. is never
    the smaller strand), which is every index the kernel can form at that k."""
    recs = table_records(k)
    assert all(len(r) == k for r in recs)
    if k <= 7:
        assert len(set(recs)) == 4 ** k
        # a genome holds at most 8192 records, below s: tau = 2^64 - 1
        s = 12000
        genomes = [recs[i:i + 8192] for i in range(0, len(recs), 8192)]
    else:
        want = {(q, u) for q in range(n_groups(k)) for u in group_patterns(k, q)}
        seen = covered_pairs(recs, k)
        assert len(want) == 256 * (k // 4) + (4 ** (k % 4) if k % 4 else 0)
        assert seen == want, (k, sorted(want - seen)[:8])
        assert all(canonical(r) == r for r in recs)
        s = 4096
        genomes = [recs]
    assert max(len(g) for g in genomes) <= s
    sk, lens = check(genomes, k, s, seed)
    if k <= 7:
        assert len(genomes) == (2 if k == 7 else 1)
        assert len(set(int(x) for g in range(len(genomes)) for x in sk[g][:lens[g]])) == N_CANONICAL[k]
    else:
        assert int(lens[0]) == len(set(recs))  # (self-canonical and distinct: no two share a hash)


def partial_group_indices(pk, k):
    """The 8-bit table indices K1 forms for the partial last group (k % 4
    valid bases) over the packed genomes `pk`: the group's valid bases of the
    canonical k-mer, then whatever follows the k-mer in the lane's 64-base
    window (sketch.hip: the forward window holds the stream from the segment's
    first base on, zeros past the buffer; the reverse-complement window ends
    at the segment's first base, zeros after)."""
    nb = k % 4
    L = seg_len(k)
    n_stream = int(pk.n_words) * 16
    stream = np.frombuffer(unpack_run(pk.words, 0, n_stream), np.uint8) if n_stream else np.zeros(0, np.uint8)
    code = np.zeros(256, np.uint8)
    code[list(b"ACGT")] = (0, 1, 2, 3)
    stream = code[stream]
    seen = set()
    for run in pk.runs:
        base, length = int(run["base"]), int(run["len"])
        for p in range(length - k + 1):
            b = base + p
            ws = b - p % L  # first base of the lane's window
            fwd = stream[b:b + k]
            rev = (3 - fwd)[::-1]
            f_tail = [int(stream[x]) if x < min(ws + 64, n_stream) else 0 for x in range(b + k, b + k + 4 - nb)]
            r_tail = [3 - int(stream[x]) if x >= ws else 0 for x in range(b - 1, b - 1 - (4 - nb), -1)]
            cands = [(tuple(fwd), tuple(f_tail)), (tuple(rev), tuple(r_tail))]
            kmer, tail = min(cands)
            idx = 0
            for c in kmer[k - nb:] + tail:
                idx = idx * 4 + int(c)
            seen.add(idx)
    return seen


@pytest.mark.parametrize("k", range(1, 33))
def test_bits_below_a_partial_last_group(k):
    """A one-k-mer record leaves the bits below a partial last group to
    whatever follows in the packed stream; 40 records of k .. k + 3L bases make
    them vary (group_term masks them out: the entries that differ only there
    hold equal values).  s is above the k-mer count, so every hash is compared.
    The share of the group's 256 indices that were formed is reported in the
    assertion message, without a threshold."""
    rng = np.random.default_rng(500 + k)
    L = seg_len(k)
    recs = tuple(rnd(rng, int(rng.integers(k, k + 3 * L + 1))) for _ in range(40))
    s = 6000
    n_kmers = sum(len(r) - k + 1 for r in recs)
    assert n_kmers < s
    note = "no partial group"
    if k % 4:
        pk = ga.pack_records([recs], k=k)
        seen = partial_group_indices(pk, k)
        note = "partial group %d (%d bases): %d of 256 indices formed" % (n_groups(k) - 1, k % 4, len(seen))
    check([recs], k, s, 0, note)


@pytest.mark.parametrize("k", range(1, 6))
def test_fewer_distinct_kmers_than_s(k):
    """k <= 5 at s = 1000: a genome holds at most 2, 10, 32, 136, 512 distinct
    canonical k-mers, so tau climbs to 2^64 - 1, where every k-mer is a
    candidate and the first pass's list outgrows its region (set mode).  A
    20,000-base random genome holds them all; a 300,000-base homopolymer (of
    T: the reverse strand is the canonical one; and of A) holds one."""
    rng = np.random.default_rng(600 + k)
    genomes = [(rnd(rng, 20000),), (b"T" * 300000,), (b"A" * 300000,)]
    with ga.Context(k=k, sketch_size=1000, seed=0) as ctx:
        sk, lens = ctx.sketch(ga.pack_records(genomes, k=k))
        fb = ctx.fallbacks()
    for g, recs in enumerate(genomes):
        exp = oracle.sketch_records(list(recs), k=k, s=1000, seed=0)
        assert lens[g] == len(exp), (k, g, int(lens[g]), len(exp))
        assert (sk[g][:lens[g]] == exp).all(), (k, g)
    assert [int(x) for x in lens] == [N_CANONICAL[k], 1, 1]
    assert sk[1][0] == sk[2][0] == murmur3_x64_128(b"A" * k)[0]
    assert fb["sketch_retry"] > 0 and fb["sketch_set"] > 0, fb
    if k % 2 == 0:  # the k-mers that are their own reverse complement
        pal = [h + revcomp(h) for h in all_kmers(k // 2)]
        assert len(pal) == 4 ** (k // 2) and all(revcomp(p) == p for p in pal)
        got = set(int(x) for x in sk[0][:lens[0]])
        assert all(murmur3_x64_128(p)[0] in got for p in pal), k
