"""The CPU oracle (oracle/finch_oracle.c) is the reference of every K1 test
at every k, but only the published murmur3 vectors and 21-mers pin it
(test_oracle_golden.py).  Here it is compared, at every k in 1..32 and two
seeds, with a plain restatement that shares nothing with it: murmurhash3_x64_128
on Python ints, the canonical form as the smaller of two byte strings, k-mers
broken at non-ACGT bytes, the sorted distinct hashes cut at s.  No GPU.
"""
import itertools
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLD

M64 = (1 << 64) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
SEEDS = (0, 12345)
# canonical k-mers among all 4^k: half of them, and the palindromes (even k) once more
N_CANONICAL = {1: 2, 2: 10, 3: 32, 4: 136, 5: 512, 6: 2080, 7: 8192}

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def fmix(k):
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & M64
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & M64
    return k ^ (k >> 33)


def murmur3_x64_128(data, seed=0):
    """MurmurHash3_x64_128 (Appleby, public domain), both halves; the 32-bit
    seed starts h1 and h2."""
    h1 = h2 = seed
    n = len(data)
    for b in range(n // 16):
        k1 = int.from_bytes(data[16 * b:16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8:16 * b + 16], "little")
        k1 = rotl(k1 * C1 & M64, 31) * C2 & M64
        h1 = ((rotl(h1 ^ k1, 27) + h2) * 5 + 0x52DCE729) & M64
        k2 = rotl(k2 * C2 & M64, 33) * C1 & M64
        h2 = ((rotl(h2 ^ k2, 31) + h1) * 5 + 0x38495AB5) & M64
    tail = data[n // 16 * 16:]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        h2 ^= rotl(k2 * C2 & M64, 33) * C1 & M64
    if tail:
        k1 = int.from_bytes(tail[:8], "little")
        h1 ^= rotl(k1 * C1 & M64, 31) * C2 & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = fmix(h1), fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


def revcomp(kmer):
    return kmer.translate(_COMP)[::-1]


def canonical(kmer):
    return min(kmer, revcomp(kmer))


def kmers(records, k):
    """Every window of k A/C/G/T bytes inside a record."""
    for r in records:
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(c in b"ACGT" for c in w):
                yield w


def restated_sketch(records, k, s, seed=0):
    hashes = {murmur3_x64_128(canonical(w), seed)[0] for w in kmers(records, k)}
    return np.array(sorted(hashes)[:s], dtype=np.uint64)


def all_kmers(k):
    return [bytes(t) for t in itertools.product(b"ACGT", repeat=k)]


def rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def test_restatement_on_published_vectors():
    """The restatement itself against the vectors that pin the oracle
    (tests/golden/murmur3_kat.json), and against the oracle's murmur3 on
    inputs of every tail shape with both seeds."""
    with open(os.path.join(GOLD, "murmur3_kat.json")) as f:
        kat = json.load(f)
    for e in kat["published"]:
        assert murmur3_x64_128(e["input"].encode()) == (e["h1"], e["h2"]), e
    for e in kat["kmers21"]:
        assert murmur3_x64_128(e["kmer"].encode())[0] == e["h1"], e
    for data in [b"x" * n for n in range(0, 41)]:
        for seed in SEEDS:
            assert murmur3_x64_128(data, seed) == oracle.murmur3_x64_128(data, seed), (data, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_equals_restatement_at_every_k(seed):
    """Records of k, k + 1, 77 and 200 random bases and one holding an N, as
    one genome and each alone, cut at s = 50 (below the k-mer count) and
    uncut."""
    for k in range(1, 33):
        rng = np.random.default_rng(1000 * seed + k)
        with_n = bytearray(rnd(rng, 120))
        with_n[int(rng.integers(k, 120 - k))] = ord("N")
        records = [rnd(rng, k), rnd(rng, k + 1), rnd(rng, 77), rnd(rng, 200), bytes(with_n)]
        for recs in [records] + [[r] for r in records]:
            for s in (50, 1000):
                exp = restated_sketch(recs, k, s, seed)
                got = oracle.sketch_records(recs, k=k, s=s, seed=seed)
                assert got.dtype == np.uint64 and len(got) == len(exp) and (got == exp).all(), (k, s, seed, recs)
        # the N breaks its record into two runs: fewer k-mers than an unbroken record
        assert len(list(kmers([bytes(with_n)], k))) == 120 - k + 1 - k


@pytest.mark.parametrize("seed", SEEDS)
def test_every_kmer_of_small_k(seed):
    """All 4^k k-mers as one-k-mer records at s = 12000: every canonical k-mer's
    hash, and as many of them as there are canonical k-mers."""
    for k, n in N_CANONICAL.items():
        recs = all_kmers(k)
        assert len(recs) == 4 ** k
        got = oracle.sketch_records(recs, k=k, s=12000, seed=seed)
        exp = restated_sketch(recs, k, 12000, seed)
        assert len(got) == n, (k, seed, len(got))
        assert len(exp) == n and (got == exp).all(), (k, seed)
