"""Inputs of the clustering tests (test_cluster.py on the CPU,
test_cluster_gpu.py on the GPU), each built once, with the expected rep_of
from the reference restatement (cluster_ref.py) or, where that restatement's
per-genome scan of all representatives would take minutes (the 20,000-vertex
paths), from the closed form the rules give.

A case is (n, pairs [k, 2] u32, ani [k] f32, T f32, expected rep_of [n] u32).
"""
import functools
import os

import numpy as np

from cluster_ref import cluster_ref
from conftest import GOLD, load_golden_pairs

GOLDEN_MIN_ANI = ("0.9", "0.0")
GOLDEN_T = ("0.9", "0.95", "0.97", "0.98", "0.99", "0.995")


def _case(n, pairs, ani, T, expected=None):
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    ani = np.asarray(ani, dtype=np.float32)
    T = np.float32(T)
    if expected is None:
        expected = cluster_ref(n, pairs.tolist(), ani, T)
    return n, pairs, ani, T, np.asarray(expected, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def golden_rows():
    """{(min_ani, cluster_ani): rep_of} of tests/golden/clusters_finch.tsv."""
    out = {}
    with open(os.path.join(GOLD, "clusters_finch.tsv")) as f:
        next(f)
        for line in f:
            m, t, reps = line.split()
            out[(m, t)] = np.array([int(x) for x in reps.split(",")], dtype=np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def golden_cache(min_ani):
    """The golden pair table cut at min_ani -> (pairs, ani)."""
    rows = [(i, j, a) for (i, j, c, t, a) in load_golden_pairs()
            if np.float64(a) >= np.float64(np.float32(min_ani))]
    return (np.array([(i, j) for i, j, _ in rows], dtype=np.uint32).reshape(-1, 2),
            np.array([a for _, _, a in rows], dtype=np.float32))


def golden_case(min_ani, T):
    pairs, ani = golden_cache(min_ani)
    return _case(27, pairs, ani, T, golden_rows()[(min_ani, T)])


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> case; expected rep_of written out by hand, and checked against
    the restatement in test_cluster.py."""
    c = {}
    c["no_genomes"] = _case(0, [], [], 0.95, [])
    c["one_genome"] = _case(1, [], [], 0.95, [0])
    c["no_pairs"] = _case(5, [], [], 0.95, [0, 1, 2, 3, 4])
    c["two_components"] = _case(4, [(0, 1), (2, 3)], [0.99, 0.99], 0.95, [0, 0, 2, 2])
    # 1 is a member (0), so 2 is a representative, and 1 is closer to 2: it joins the higher index
    c["three_genomes"] = _case(3, [(0, 1), (1, 2)], [0.96, 0.97], 0.95, [0, 2, 2])
    # 2 has the same f32 ANI to representatives 0 and 1 (no pair between them): the smaller wins;
    # the larger comes first in the input
    c["tie_smaller_rep"] = _case(3, [(1, 2), (2, 0)], [0.97, 0.97], 0.95, [0, 1, 0])
    c["threshold_above_all"] = _case(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [0.9, 0.91, 0.92, 0.93], 0.99,
                                     [0, 1, 2, 3])
    # every pair strong: 0 rep, 1 member, 2 rep (its only strong lower neighbour is a member), 3 member
    c["threshold_below_all"] = _case(4, [(0, 1), (1, 2), (2, 3)], [0.8, 0.8, 0.8], 0.5, [0, 0, 2, 2])
    # 3 is made a member by its strong lower neighbour 0 (0.96); its best representative, 4 (0.98),
    # is not among its strong lower neighbours (a higher index), and the representative 1, a weak
    # neighbour (0.90 < T), does not win.  A weak pair cannot beat a strong one: strong is ani >= T.
    c["best_rep_not_a_strong_lower_neighbour"] = _case(
        5, [(0, 3), (1, 3), (3, 4), (2, 3), (0, 2)], [0.96, 0.90, 0.98, 0.97, 0.96], 0.95, [0, 1, 0, 4, 4])
    # an equality at the threshold is strong (>=, f32 against f32)
    t = np.float32(0.95)
    c["equal_to_threshold"] = _case(2, [(0, 1)], [t], t, [0, 0])
    c["just_below_threshold"] = _case(2, [(0, 1)], [np.nextafter(t, np.float32(0))], t, [0, 1])
    return c


PATH_N = 20000


@functools.lru_cache(maxsize=None)
def path_case(rising):
    """The path (i, i + 1), every pair strong.  One ANI value: the
    representatives are the even indices and odd i joins i - 1 (the tie goes
    to the smaller).  ANI rising along the path: odd i joins i + 1 (the last
    vertex, odd, has only i - 1)."""
    n = PATH_N
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.uint32)
    if rising:
        ani = (np.float32(0.96) + np.arange(n - 1, dtype=np.float32) * np.float32(1e-6)).astype(np.float32)
        assert (np.diff(ani) > 0).all()
    else:
        ani = np.full(n - 1, 0.97, dtype=np.float32)
    g = np.arange(n, dtype=np.uint32)
    exp = np.where(g % 2 == 0, g, g + 1 if rising else g - 1).astype(np.uint32)
    exp[n - 1] = n - 2  # (n even: the last vertex is odd)
    return _case(n, pairs, ani, 0.95, exp)


CLIQUE_N = 1500


@functools.lru_cache(maxsize=None)
def clique_case():
    """All pairs of 1,500 genomes strong (1,124,250 pairs): one representative;
    the last vertex has 1,499 strong lower neighbours."""
    n = CLIQUE_N
    i, j = np.triu_indices(n, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    rng = np.random.default_rng(7)
    ani = rng.choice(np.array([0.96, 0.97, 0.98], dtype=np.float32), size=len(pairs))
    return _case(n, pairs, ani, 0.95, np.zeros(n, dtype=np.uint32))


ANI_VALUES = np.array([0.90, 0.93, 0.949999, 0.95, 0.950001, 0.96, 0.97, 0.99], dtype=np.float32)
RANDOM_SHAPES = ((40, 200), (300, 2000), (700, 9000), (1500, 50000), (3000, 12000), (5000, 40000))


def _random_pairs(rng, n, m):
    a = rng.integers(0, n, size=m, dtype=np.int64)
    b = rng.integers(0, n, size=m, dtype=np.int64)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    _, first = np.unique(lo * n + hi, return_index=True)  # each unordered pair once
    first.sort()
    lo, hi = lo[first], hi[first]
    flip = rng.random(len(lo)) < 0.5  # either orientation, in the order drawn
    return np.stack([np.where(flip, hi, lo), np.where(flip, lo, hi)], axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """n <= 5,000 genomes, up to 50,000 pairs, the ANI from eight f32 values
    around the threshold so that ties are common."""
    rng = np.random.default_rng(1000 + seed)
    n, m = RANDOM_SHAPES[seed]
    pairs = _random_pairs(rng, n, m)
    return _case(n, pairs, rng.choice(ANI_VALUES, size=len(pairs)), 0.95)


@functools.lru_cache(maxsize=None)
def boundary_case():
    """A little more than the 1,024 vertices one workgroup sweeps: random
    pairs plus a strong path over 990 .. 1060, so that chains of decisions
    cross the boundary between the first range and the second."""
    rng = np.random.default_rng(99)
    n = 1100
    rand = _random_pairs(rng, n, 6000)
    chain = {(i, i + 1) for i in range(990, 1060)}
    rand = np.array([p for p in rand.tolist() if (min(p), max(p)) not in chain], dtype=np.uint32).reshape(-1, 2)
    pairs = np.concatenate([rand, np.array(sorted(chain), dtype=np.uint32)])
    ani = np.concatenate([rng.choice(ANI_VALUES, size=len(rand)), np.full(len(chain), 0.97, dtype=np.float32)])
    return _case(n, pairs, ani.astype(np.float32), 0.95)
