"""K1's window loop (sketch.hip): a lane hashes kStretch consecutive segments
per visit and carries its place in the run from window to window.  Everything
here goes through the public path (pack_records, Context.sketch) and is
compared with the CPU oracle bit for bit, on the smallest shapes at which the
loop can go wrong:
k-mer counts around the segment, stretch and workgroup-visit edges, stretches
that cross runs and genomes, every funnel offset at the end of the packed
buffer, other k, several K1 launches and a set-mode retry pass.  Needs an
MI355X.
"""
import functools

import numpy as np
import pytest

import galah_amd as ga
import oracle

pytestmark = pytest.mark.gpu

# kStretch of sketch.hip; the edge sizes are taken for 2 and 4 both, so the
# cases keep their point if the constant is retuned between the two
STRETCHES = (2, 4)
K1_BLOCK = 256  # kBlock of sketch.hip


def seg_len(k):
    """k1_seg_len(k, 4) of gg_internal.hpp: the k-mers of a 64-base window,
    65 - k, rounded down to a multiple of the tau-branch group of 4 and capped
    at 48.  48 for k <= 17, 44 for k = 18..21, 40 for 22..25, 36 for 26..29,
    32 for 30..32."""
    return min((65 - k) // 4 * 4, 48)


def rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def check(genomes, k=21, s=1000, seed=0, ctx=None):
    """Sketch `genomes` (lists of records) in one call and compare every row with the oracle."""
    def run(c):
        sk, lens = c.sketch(ga.pack_records(genomes, k=k))
        for g, recs in enumerate(genomes):
            exp = expected(tuple(recs), k, s, seed)
            assert lens[g] == len(exp), (k, s, seed, g, int(lens[g]), len(exp))
            assert (sk[g][:lens[g]] == exp).all(), (k, s, seed, g)
    if ctx is not None:
        return run(ctx)
    with ga.Context(k=k, sketch_size=s, seed=seed) as c:
        run(c)


@functools.lru_cache(maxsize=None)
def expected(recs, k, s, seed):
    out = oracle.sketch_records(list(recs), k=k, s=s, seed=seed)
    out.setflags(write=False)
    return out


def edge_counts(k):
    """K-mer counts around one segment, one stretch and one visit of a workgroup."""
    L = seg_len(k)
    ns = {1, L - 1, L, L + 1}
    for S in STRETCHES:
        ns |= {S * L - 1, S * L, S * L + 1, K1_BLOCK * S * L - 1, K1_BLOCK * S * L, K1_BLOCK * S * L + 1}
    return sorted(ns)


@functools.lru_cache(maxsize=None)
def edge_genomes(k):
    """One single-record genome per count of edge_counts(k)."""
    rng = np.random.default_rng(100 + k)
    return tuple((rnd(rng, n + k - 1),) for n in edge_counts(k))


@functools.lru_cache(maxsize=None)
def crossing_genomes(k):
    """~300 genomes of 1-7 records of k .. k + 3L bases, a few records with an
    N (their runs split), one genome with no record: stretches cross one or
    more run and genome boundaries and meet another tau and slot midway."""
    rng = np.random.default_rng(200 + k)
    L = seg_len(k)
    genomes = []
    for g in range(300):
        recs = []
        for _ in range(int(rng.integers(1, 8))):
            r = bytearray(rnd(rng, int(rng.integers(k, k + 3 * L + 1))))
            if rng.random() < 0.05:
                r[int(rng.integers(0, len(r)))] = ord("N")
            recs.append(bytes(r))
        genomes.append(tuple(recs))
    genomes[150] = ()
    return tuple(genomes)


def test_kmer_counts_around_stretch_edges():
    """Single-record genomes of 1, L-1, L, L+1, S L-1 .. 256 S L+1 k-mers, each
    sketched alone (below 1000 k-mers the sketch is every distinct hash, so a
    dropped or doubled window shows) and all in one call."""
    genomes = edge_genomes(21)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        for g in genomes:
            check([g], ctx=ctx)
        check(list(genomes), ctx=ctx)


def test_stretches_cross_runs_and_genomes():
    check(list(crossing_genomes(21)))


@pytest.mark.parametrize("off", range(16))
def test_funnel_offsets_at_buffer_end(off):
    """The last record starts at base `off` mod 16 and ends the packed
    buffer: its last windows reach past the buffer's last word and must read
    the words past it as zeros."""
    rng = np.random.default_rng(300 + off)
    L = seg_len(21)
    genome = (rnd(rng, 32 + off), rnd(rng, 21 - 1 + L + 1 + off % 5))
    pk = ga.pack_records([genome])
    assert int(pk.runs[-1]["base"]) % 16 == off and int(pk.n_words) == (sum(map(len, genome)) + 15) // 16
    check([genome])


OTHER_K = ([(k, 500, 0) for k in range(1, 33) if k != 21] + [(k, 50, 0) for k in (5, 16, 31, 32)] +
           [(16, 500, 12345), (22, 500, 12345)])


@pytest.mark.parametrize("k,s,seed", OTHER_K)
def test_other_k(k, s, seed):
    """Every k the kernel is compiled for but 21 (the tests above).  The
    segment is L = min(4 * ((65 - k) // 4), 48) k-mers: 48 up to k = 17, 44 at
    k = 18..21, 40 at 22..25, 36 at 26..29 and 32 at 30..32, and the k-mer's
    place in the lane's window takes another shift branch of window64 at every
    k.  Below k = 5 a genome holds fewer distinct k-mers than s, so tau climbs
    to 2^64 - 1.  Two cases with a non-zero seed (the kernel variant that keeps
    the seed terms): k = 16, one murmur block and no tail, and k = 22, a block
    and a tail of two group tables."""
    with ga.Context(k=k, sketch_size=s, seed=seed) as ctx:
        check(list(edge_genomes(k)), k, s, seed, ctx=ctx)
        check(list(crossing_genomes(k)), k, s, seed, ctx=ctx)


def test_batches_of_two(monkeypatch):
    """GALAHGPU_K1_MAX_BATCH=2: one K1 launch per two genomes, each from its
    own first segment (seg0 != 0) over its slice of the run index."""
    monkeypatch.setenv("GALAHGPU_K1_MAX_BATCH", "2")
    check(list(crossing_genomes(21)))


@pytest.mark.parametrize("max_batch", ["0", "2"])
def test_set_mode_retry_pass(monkeypatch, max_batch):
    """Tandem repeats outgrow the append list, so those genomes are hashed
    again in set mode: a retry pass over a subset of the genomes."""
    rng = np.random.default_rng(13)
    genomes = [(rnd(rng, 5000) * 40,), (rnd(rng, 50000),), (rnd(rng, 20000) * 10, rnd(rng, 3000))]
    monkeypatch.setenv("GALAHGPU_K1_MAX_BATCH", max_batch)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        check(genomes, ctx=ctx)
        fb = ctx.fallbacks()
        assert fb["sketch_set"] >= 2 and fb["sketch_retry"] > 0, fb


def test_contexts_of_different_k():
    """Two contexts with different k on one device each hash with their own
    murmur tables: k = 21, then 31, then 21 again, the contexts alive together."""
    rng = np.random.default_rng(17)
    genomes = [(rnd(rng, 30000),), (rnd(rng, 500), rnd(rng, 77))]
    with ga.Context(k=21, sketch_size=1000) as c21, ga.Context(k=31, sketch_size=1000) as c31:
        check(genomes, 21, ctx=c21)
        check(genomes, 31, ctx=c31)
        check(genomes, 21, ctx=c21)
    with ga.Context(k=21, sketch_size=1000) as again:
        check(genomes, 21, ctx=again)
