"""The finch + finch clustering step on the host, CPU only:
gg_cluster_pairs_host and gg_clusters_from_reps against the restatement of
the reference's two loops (tests/cluster_ref.py: src/clusterer.rs:155-225 and
:316-406 with skip_clusterer), on the inputs of tests/cluster_cases.py.  The
same inputs go through the device path in test_cluster_gpu.py."""
import ctypes

import numpy as np
import pytest

import cluster_cases as cc
import galah_amd as ga
from cluster_ref import cluster_ref, clusters_ref

GG_ERR_INVALID_ARG = 1


def check_host(case):
    n, pairs, ani, T, exp = case
    got = ga.cluster_pairs_host(n, pairs, ani, T)
    assert got.dtype == np.uint32 and got.tolist() == exp.tolist()
    assert ga.clusters_from_reps(got) == clusters_ref(exp)


@pytest.mark.parametrize("T", cc.GOLDEN_T)
@pytest.mark.parametrize("min_ani", cc.GOLDEN_MIN_ANI)
def test_golden_pairs(min_ani, T):
    case = cc.golden_case(min_ani, T)
    n, pairs, ani, thr, exp = case
    assert len(pairs) == (161 if min_ani == "0.9" else 351)
    # the committed rows are what the restatement gives today
    assert cluster_ref(n, pairs.tolist(), ani, thr).tolist() == exp.tolist()
    check_host(case)


def test_golden_cluster_counts_and_backward_members():
    for m in cc.GOLDEN_MIN_ANI:
        counts, backward = [], []
        for T in cc.GOLDEN_T:
            rep_of = ga.cluster_pairs_host(*cc.golden_case(m, T)[:4])
            counts.append(len(ga.clusters_from_reps(rep_of)))
            backward.append(int(sum(int(r) > g for g, r in enumerate(rep_of))))
        assert counts == [5, 5, 7, 10, 16, 21]
        # members whose representative has the higher index: what a forward-only pass gets wrong
        assert backward == [0, 0, 1, 5, 1, 0]


@pytest.mark.parametrize("name", sorted(cc.hand_cases()))
def test_hand_graphs(name):
    case = cc.hand_cases()[name]
    n, pairs, ani, T, exp = case
    assert cluster_ref(n, pairs.tolist(), ani, T).tolist() == exp.tolist()  # the hand-written answer
    check_host(case)


def test_pairs_reversed_and_shuffled():
    n, pairs, ani, T, exp = cc.golden_case("0.0", "0.98")
    rng = np.random.default_rng(5)
    order = rng.permutation(len(pairs))
    flipped = pairs[order][:, ::-1].copy()
    assert ga.cluster_pairs_host(n, flipped, ani[order], T).tolist() == exp.tolist()
    # a structured PAIR_DTYPE array, as precluster_files returns it
    p = np.zeros(len(pairs), ga.PAIR_DTYPE)
    p["i"], p["j"] = pairs[:, 0], pairs[:, 1]
    assert ga.cluster_pairs_host(n, p, ani, T).tolist() == exp.tolist()


def test_invalid_arguments():
    ok_pairs, ok_ani = [(0, 1), (1, 2)], [0.96, 0.97]
    assert ga.cluster_pairs_host(3, ok_pairs, ok_ani, 0.95).tolist() == [0, 2, 2]
    bad = [
        (3, [(0, 1), (1, 3)], ok_ani, 0.95),          # an index >= n
        (3, [(0, 1), (2, 2)], ok_ani, 0.95),          # i == j
        (3, ok_pairs, [0.96, float("nan")], 0.95),    # a NaN ANI
        (3, ok_pairs, ok_ani, float("nan")),          # a NaN threshold
    ]
    for n, pairs, ani, T in bad:
        with pytest.raises(ga.GalahGpuError) as e:
            ga.cluster_pairs_host(n, pairs, ani, T)
        assert e.value.status == GG_ERR_INVALID_ARG
    # n_pairs >= 2^31: refused before a pair is read
    p = np.zeros(2, ga.PAIR_DTYPE)
    a = np.zeros(2, np.float32)
    out = np.zeros(3, np.uint32)
    st = ga.lib().gg_cluster_pairs_host(3, p.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p),
                                        1 << 31, ctypes.c_float(0.95), out.ctypes.data_as(ctypes.c_void_p))
    assert st == GG_ERR_INVALID_ARG
    with pytest.raises(ga.GalahGpuError):
        ga.clusters_from_reps([1, 2, 2])  # 0 -> 1, which is not a representative
    with pytest.raises(ga.GalahGpuError):
        ga.clusters_from_reps([0, 5])


@pytest.mark.parametrize("rising", (False, True))
def test_path_graphs(rising):
    case = cc.path_case(rising)
    n, pairs, ani, T, exp = case
    # the closed form, checked against the restatement on the path's first 400 vertices
    m = 400
    head = cluster_ref(m, pairs[:m - 1].tolist(), ani[:m - 1], T)
    assert head[:m - 1].tolist() == exp[:m - 1].tolist()
    check_host(case)
    got = ga.cluster_pairs_host(n, pairs, ani, T)
    assert (got[::2] == np.arange(0, n, 2)).all()
    assert (got[1:n - 1:2] == np.arange(1, n - 1, 2) + (1 if rising else -1)).all()


def test_clique():
    case = cc.clique_case()
    assert len(case[1]) == cc.CLIQUE_N * (cc.CLIQUE_N - 1) // 2
    check_host(case)
    assert ga.clusters_from_reps(ga.cluster_pairs_host(*case[:4])) == [list(range(cc.CLIQUE_N))]


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs(seed):
    case = cc.random_case(seed)
    n, pairs, ani, T, exp = case
    assert n <= 5000 and len(pairs) <= 50000
    assert len(set(exp.tolist())) not in (1, n)  # both representatives and members
    check_host(case)


def test_boundary_graph():
    check_host(cc.boundary_case())


def test_clusters_from_reps_order():
    assert ga.clusters_from_reps([]) == []
    assert ga.clusters_from_reps([0]) == [[0]]
    # by representative ascending, the representative first, then members ascending
    assert ga.clusters_from_reps([3, 1, 3, 3, 1, 5]) == [[1, 4], [3, 0, 2], [5]]
