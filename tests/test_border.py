"""Adding genomes to a finished run, the parts that need no device (DESIGN.md
4.7): gg_pairs_border_host against the CPU oracle, the argument checks,
PreclusterState on disk, and the relabelling of pairs under an order."""
import functools
import io

import numpy as np
import pytest

import galah_amd as ga
import oracle
from test_gpu_parity import adversarial_sketches, random_sketch_set

f32 = np.float32
N, S = 200, 32
N_OLD = (0, 1, 64, 199, 200)
THRESHOLDS = (0.0, 0.9, 1.0)


def quads(p):
    return np.stack([p["i"], p["j"], p["common"], p["total"]], axis=1).astype(np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def rows(kind):
    if kind == "random":
        sk, lens = random_sketch_set(np.random.default_rng(41), N, S, 4)
    else:
        sk, lens = adversarial_sketches(np.random.default_rng(43), N, S)
    # every pair once, from the oracle (the thresholds filter it below)
    allp = quads(oracle.pairs(sk, lens.astype(np.int32), f32(0.0)))
    assert len(allp) == N * (N - 1) // 2
    u, inv = np.unique(allp[:, 2:], axis=0, return_inverse=True)
    ani = oracle.ani_array(u[:, 0], u[:, 1], 21)[inv.reshape(-1)]
    for a in (sk, lens, allp, ani):
        a.setflags(write=False)
    return sk, lens, allp, ani


@pytest.mark.parametrize("kind", ["random", "adversarial"])
def test_pairs_border_host_matches_the_oracle(kind):
    sk, lens, allp, ani = rows(kind)
    for thr in THRESHOLDS:
        passing = allp[ani >= np.float64(f32(thr))]
        # the filter is the oracle's own answer at this threshold
        assert (quads(oracle.pairs(sk, lens.astype(np.int32), f32(thr))) == passing).all()
        if thr > 0:  # (the adversarial rows hold identical ones, which pass at 1.0)
            assert len(passing) < len(allp) and (len(passing) > 0 or kind == "random")
        for n_old in N_OLD:
            exp = passing[passing[:, 1] >= n_old]
            got = quads(ga.pairs_border_host(sk, lens, n_old, f32(thr)))
            assert got.shape == exp.shape and (got == exp).all(), (kind, thr, n_old)
            if n_old == N:
                assert len(got) == 0
            # the contract: the old pairs and the border are the whole, disjoint
            old = quads(ga.pairs_border_host(sk[:n_old], lens[:n_old], 0, f32(thr)))
            both = np.concatenate([old, got])
            assert len(np.unique(both[:, :2], axis=0)) == len(both) == len(passing), (kind, thr, n_old)


def test_pairs_border_host_other_k():
    sk, lens, allp, _ = rows("random")
    u, inv = np.unique(allp[:, 2:], axis=0, return_inverse=True)
    ani = oracle.ani_array(u[:, 0], u[:, 1], 2)[inv.reshape(-1)]
    exp = allp[(ani >= np.float64(f32(0.5))) & (allp[:, 1] >= 150)]
    assert 0 < len(exp)
    assert (quads(ga.pairs_border_host(sk, lens, 150, f32(0.5), k=2)) == exp).all()


def test_argument_errors():
    sk, lens, _, _ = rows("random")
    with pytest.raises(ga.GalahGpuError) as e:
        ga.pairs_border_host(sk, lens, N + 1, 0.9)
    assert e.value.status == 1 and "n_old" in str(e.value)
    with pytest.raises(ga.GalahGpuError) as e:
        ga.pairs_border_host(sk, lens, 10, float("nan"))
    assert e.value.status == 1
    with pytest.raises(ga.GalahGpuError) as e:
        ga.pairs_border_host(sk, lens, 10, 0.9, k=33)
    assert e.value.status == 1
    long = lens.copy()
    long[7] = S + 1
    with pytest.raises(ga.GalahGpuError) as e:
        ga.pairs_border_host(sk, long, 10, 0.9)
    assert e.value.status == 1 and "sketch_size" in str(e.value)
    with pytest.raises(ValueError):
        ga.pairs_border_host(sk[:, :5].reshape(-1), lens, 10, 0.9)
    assert len(ga.pairs_border_host(np.zeros((0, S), np.uint64), np.zeros(0, np.uint32), 0, 0.9)) == 0


def make_state():
    sk, lens, allp, ani = rows("random")
    keep = ani >= 0.9
    pairs = np.zeros(int(keep.sum()), ga.PAIR_DTYPE)
    for x, f in enumerate(("i", "j", "common", "total")):
        pairs[f] = allp[keep][:, x]
    paths = ["dir/g%03d.fna" % g for g in range(N - 1)] + ["café/\udcff.fna"]  # (a non-UTF-8 file name)
    return ga.PreclusterState(paths, sk, lens, pairs, ani[keep].astype(f32), 21, S, 0, f32(0.9))


def assert_same_state(a, b):
    assert a.paths == b.paths
    assert a.sketches.dtype == b.sketches.dtype == np.uint64 and (a.sketches == b.sketches).all()
    assert a.lens.dtype == b.lens.dtype == np.uint32 and (a.lens == b.lens).all()
    assert a.pairs.dtype == b.pairs.dtype == ga.PAIR_DTYPE and (a.pairs == b.pairs).all()
    assert a.ani.dtype == b.ani.dtype == np.float32 and (a.ani.view(np.uint32) == b.ani.view(np.uint32)).all()
    assert (a.k, a.s, a.seed) == (b.k, b.s, b.seed)
    assert f32(a.min_ani).tobytes() == f32(b.min_ani).tobytes()


def test_precluster_state_round_trip(tmp_path):
    st = make_state()
    assert len(st.pairs) > 0
    p = tmp_path / "state.npz"
    st.save(p)
    assert_same_state(ga.PreclusterState.load(p), st)
    with np.load(p, allow_pickle=False) as z:  # data only: every member loads without pickle
        assert all(z[name].dtype != object for name in z.files)
    buf = io.BytesIO()
    st.save(buf)
    buf.seek(0)
    assert_same_state(ga.PreclusterState.load(buf), st)
    cache = st.cache()
    assert isinstance(cache, ga.SortedPairGenomeDistanceCache) and len(cache) == len(st.pairs)
    r = st.pairs[0]
    assert cache.get((int(r["j"]), int(r["i"]))) == st.ani[0]
    empty = ga.PreclusterState([], np.zeros((0, S), np.uint64), [], np.zeros(0, ga.PAIR_DTYPE), [], 21, S, 0, 0.95)
    empty.save(p)
    assert_same_state(ga.PreclusterState.load(p), empty)
    assert len(empty.cache()) == 0


def test_update_refuses_a_mismatched_state_or_a_repeated_path():
    st = make_state()
    for kw in ({"min_ani": 0.95}, {"num_kmers": S + 1}, {"kmer_length": 20}):
        args = {"min_ani": 0.9, "num_kmers": S, "kmer_length": 21}
        args.update(kw)
        with pytest.raises(ValueError):
            ga.FinchPreclusterer(**args).update(st, ["new.fna"])
    seeded = ga.PreclusterState(st.paths, st.sketches, st.lens, st.pairs, st.ani, 21, S, 1, f32(0.9))
    with pytest.raises(ValueError):
        ga.FinchPreclusterer(0.9, S, 21).update(seeded, ["new.fna"])
    with pytest.raises(ValueError, match="already present"):
        ga.FinchPreclusterer(0.9, S, 21).update(st, ["new.fna", st.paths[3]])
    with pytest.raises(ValueError, match="already present"):
        ga.FinchPreclusterer(0.9, S, 21).update(st, ["new.fna", "new.fna"])


def test_relabelling_under_a_random_order():
    st = make_state()
    rng = np.random.default_rng(47)
    order = rng.permutation(N)
    got = ga.relabel_pairs(st.pairs, order)
    assert got.dtype == ga.PAIR_DTYPE and len(got) == len(st.pairs)
    # position p holds genome order[p]: a relabelled pair names the same two genomes
    assert (order[got["i"]] == st.pairs["i"]).all() and (order[got["j"]] == st.pairs["j"]).all()
    assert (got["common"] == st.pairs["common"]).all() and (got["total"] == st.pairs["total"]).all()
    assert (got["i"] > got["j"]).any() and (got["i"] < got["j"]).any()
    # clustering the relabelled pairs is clustering the genomes in that order:
    # against the all-pairs answer of the permuted rows
    sk, lens, _, _ = rows("random")
    perm = quads(oracle.pairs(sk[order], lens[order].astype(np.int32), f32(0.9)))
    lo, hi = np.minimum(got["i"], got["j"]), np.maximum(got["i"], got["j"])
    mine = np.stack([lo, hi, got["common"], got["total"]], axis=1).astype(np.uint32)
    mine = mine[np.lexsort((mine[:, 1], mine[:, 0]))]
    assert mine.shape == perm.shape and (mine == perm).all()
    ident = ga.relabel_pairs(st.pairs, np.arange(N))
    assert (ident == st.pairs).all()
    for bad in (np.arange(N - 1), np.zeros(N, np.int64), np.arange(1, N + 1)):
        with pytest.raises(ValueError):
            ga.relabel_pairs(st.pairs, bad)
