"""Inputs of the device precluster step, built once for the
CPU test of its shared rules (test_precluster_core.py) and the GPU test
(test_preclusters_gpu.py).  A case is (n_genomes, pairs): pairs a PAIR_DTYPE
array whose common and total are not read.  The shapes are the smallest at
which each part of the step can go wrong; the expected result is always what
the host forms (precluster.cpp) give for the same input."""
import functools

import numpy as np

import galah_amd as ga
import oracle
from conftest import load_golden_pairs, load_golden_sketches

PATH_N = 20000
STAR_LEAVES = 5000
CLIQUE = 300
CLIQUE_SINGLETONS = 50


def pair_array(ij):
    ij = np.asarray(ij, dtype=np.uint32).reshape(-1, 2)
    p = np.zeros(len(ij), ga.PAIR_DTYPE)
    p["i"], p["j"] = ij[:, 0], ij[:, 1]
    return p


@functools.lru_cache(maxsize=None)
def golden_case():
    """The 27 golden genomes at 0.9: 161 pairs, in the reference's order."""
    rows = [(i, j) for (i, j, c, t, a) in load_golden_pairs() if oracle.ani(c, t) >= np.float64(np.float32(0.9))]
    assert len(rows) == 161
    return 27, pair_array(rows)


@functools.lru_cache(maxsize=None)
def abisko4_case():
    """src/clusterer.rs:482-612: the 4 abisko4 genomes that make one precluster at 0.9."""
    names, _, _ = load_golden_sketches()
    want = ["abisko4/73.20120800_S1X.13.fna", "abisko4/73.20120600_S2D.19.fna",
            "abisko4/73.20120700_S3X.12.fna", "abisko4/73.20110800_S2D.13.fna"]
    pos = {names.index(w): k for k, w in enumerate(want)}
    rows = [(pos[i], pos[j]) for (i, j, c, t, a) in load_golden_pairs()
            if i in pos and j in pos and oracle.ani(c, t) >= np.float64(np.float32(0.9))]
    return 4, pair_array(rows)


def edge_cases():
    return {
        "n0": (0, pair_array([])),
        "n1": (1, pair_array([])),
        "n5_no_pairs": (5, pair_array([])),
        "size_tie": (4, pair_array([(0, 3), (1, 2)])),  # equal sizes: smallest member first
        "three_and_two": (6, pair_array([(4, 5), (0, 1), (1, 2)])),
    }


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """n up to 3,000, up to 3 n pairs; on odd seeds reversed and shuffled; some
    pairs twice, some i == j."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 3001))
    m = int(rng.integers(1, 3 * n + 1))
    ij = rng.integers(0, n, (m, 2))
    ij.sort(axis=1)
    ij = ij[np.lexsort((ij[:, 1], ij[:, 0]))]
    dup = ij[rng.integers(0, m, max(1, m // 20))]         # duplicates of pairs that are there
    same = np.repeat(rng.integers(0, n, max(1, m // 50)), 2).reshape(-1, 2)  # i == j
    ij = np.concatenate([ij, dup, same])
    if seed % 2:
        ij = ij[rng.permutation(len(ij))][:, ::-1]
    return n, pair_array(ij)


@functools.lru_cache(maxsize=None)
def path_case(shuffled):
    """0 - 1 - ... - 19,999.  In order, the hook launch may leave a chain as deep as n."""
    ij = np.stack([np.arange(PATH_N - 1), np.arange(1, PATH_N)], axis=1)
    if shuffled:
        ij = ij[np.random.default_rng(11).permutation(len(ij))]
    return PATH_N, pair_array(ij)


@functools.lru_cache(maxsize=None)
def star_case(hub_last):
    """5,000 leaves on one hub: every hook contends on one root; with the hub
    the largest index, the root moves under every compare-and-swap."""
    n = STAR_LEAVES + 1
    hub = n - 1 if hub_last else 0
    leaves = np.array([g for g in range(n) if g != hub])
    ij = np.stack([np.full(STAR_LEAVES, hub), leaves], axis=1)
    return n, pair_array(ij)


@functools.lru_cache(maxsize=None)
def cliques_case():
    """Two cliques of 300, even genomes in one and odd genomes in the other,
    then 50 singletons: equal sizes (the tie rule orders them), positions that
    differ from indices, 2 x 44,850 pairs, shuffled."""
    rows = []
    for first in (0, 1):
        v = np.arange(first, 2 * CLIQUE, 2)
        a, b = np.triu_indices(CLIQUE, 1)
        rows.append(np.stack([v[a], v[b]], axis=1))
    ij = np.concatenate(rows)
    assert len(ij) == 2 * 44850
    ij = ij[np.random.default_rng(12).permutation(len(ij))]
    return 2 * CLIQUE + CLIQUE_SINGLETONS, pair_array(ij)


@functools.lru_cache(maxsize=None)
def clusters_case():
    """10,000 genomes in 1,000 clusters of 10 (a random assignment), every
    pair inside a cluster present, shuffled: many sets of one size."""
    rng = np.random.default_rng(13)
    groups = rng.permutation(10000).reshape(1000, 10)
    a, b = np.triu_indices(10, 1)
    ij = np.stack([groups[:, a].ravel(), groups[:, b].ravel()], axis=1)
    ij = ij[rng.permutation(len(ij))]
    return 10000, pair_array(ij)


@functools.lru_cache(maxsize=None)
def width_case(n):
    """About 2 n random pairs (n = 1,025; n = 65,537: an index takes 17 bits from 65,537 on)."""
    rng = np.random.default_rng(n)
    return n, pair_array(rng.integers(0, n, (2 * n, 2)))


def all_cases():
    """{name: case}, every case above."""
    cases = {"golden": golden_case(), "abisko4": abisko4_case()}
    cases.update(edge_cases())
    for seed in range(6):
        cases["random%d" % seed] = random_case(seed)
    cases["path"], cases["path_shuffled"] = path_case(False), path_case(True)
    cases["star_hub0"], cases["star_hub_last"] = star_case(False), star_case(True)
    cases["cliques"], cases["clusters"] = cliques_case(), clusters_case()
    cases["n1025"], cases["n65537"] = width_case(1025), width_case(65537)
    return cases


@functools.lru_cache(maxsize=None)
def host_result(name):
    """What the host forms give for a case: (members, offsets, local, pair_offsets)."""
    n, pairs = all_cases()[name]
    members, offsets = ga.partition_preclusters(n, pairs)
    local, poff = ga.precluster_pairs(n, pairs, members, offsets)
    return members, offsets, local, poff
