"""The collection resident on the device: genomes added,
removed and clustered with the sketch matrix, the pair list and its ANI kept in
device memory.  Needs an MI355X.

Expected values come from the CPU oracle, numpy, tests/cluster_ref.py and the
existing from-scratch entry points on the same rows only.  Bar: (i, j, common,
total) identical and in (i, j) order, f32 ANI identical bit for bit, rows and
rep_of identical.

A  growth in pieces at tile edges, from a capacity of 1, both pairs paths
B  removal: 92 of 600 rows against the oracle on the 508 survivors, the row
   compaction in batches of 1, 7, 64 and the default; nothing, all, back again
C  a failed call leaves the collection as it was
D  cluster in three orders at thresholds below, at and above min_ani
E  files: the 27 golden genomes through ga.Collection, save / load / from_state
F  view + preclusters_device; the pair-kernel knobs give the same collection
"""
import functools
import os

import numpy as np
import pytest

import cluster_ref
import galah_amd as ga
import oracle
from test_border_gpu import CONFIGS, border_thresholds, golden_table, set_config, table_cache
from test_pair_edges import SWEEP_S, assert_pairs, pair_ani, quads, sweep_reference, sweep_rows, torch_dev

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = 0xFFFFFFFF
INVALID, IO = 1, 2
PIECES = (0, 1, 63, 64, 65, 300, 536, 599, 600)  # test_border_gpu.SWEEP_N_OLD
REMOVED = np.array(sorted({0, 63, 64, 65, 299, 300, 598, 599} | set(range(5, 600, 7))), dtype=np.uint32)


class Handle:
    """A gg_collection on ctx, destroyed on exit."""

    def __init__(self, ctx, min_ani, reserve_rows=0, reserve_pairs=0):
        self.ctx = ctx
        self.h = ctx.collection_create(float(f32(min_ani)), reserve_rows, reserve_pairs)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.collection_destroy(self.h)

    def __getattr__(self, name):
        f = getattr(self.ctx, "collection_" + name)
        return lambda *a, **k: f(self.h, *a, **k)

    def info(self):
        return self.ctx.collection_stat(self.h)[0]


def assert_collection(col, exp_q, exp_ani64, what):
    """The collection's list is exp_q ([m, 4] in (i, j) order) with the f32 of exp_ani64."""
    pairs, ani = col.pairs()
    assert_pairs(pairs, exp_q, what)
    assert ani.dtype == np.float32 and (ani.view(np.uint32) == exp_ani64.astype(np.float32).view(np.uint32)).all(), what
    info = col.info()
    assert info["n_pairs"] == len(exp_q) <= info["pair_capacity"] or len(exp_q) == 0, (what, info)


# ----------------------------------------------------------------------------
# A. growth in pieces
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 2])
@pytest.mark.parametrize("path", ["default", "matrix"])
def test_growth_in_pieces(path, k):
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(k)
    with ga.Context(k=k, sketch_size=SWEEP_S) as ctx:
        ctx.set_pairs_path(path)
        for thr in border_thresholds(v):
            passing = ani >= np.float64(thr)
            eq, ea = q[passing], ani[passing]
            assert len(eq) == 179700 if thr == 0 else 0 < len(eq) < len(q)
            with Handle(ctx, thr, reserve_rows=1, reserve_pairs=1) as col:
                taken = ctx.pairs_paths_taken()
                for a, b in zip(PIECES[:-1], PIECES[1:]):
                    added = col.add_rows(sk[a:b], lens[a:b])
                    present = eq[:, 1] < b
                    assert added == int((present & (eq[:, 1] >= a)).sum()), (thr, a, b)
                    assert_collection(col, eq[present], ea[present], "%s k=%d min_ani=%r rows %d" % (path, k, thr, b))
                    info = col.info()
                    assert info["n_rows"] == b <= info["row_capacity"], info
                assert col.add_rows(sk[:0], lens[:0]) == 0 and col.info()["n_rows"] == 600  # a no-op
                info = col.info()
                assert info["grows"] > 0 and info["device_bytes"] >= 600 * (SWEEP_S * 8 + 4) + 20 * len(eq), info
                rows, rlens = col.rows()
                assert (rows == sk).all() and (rlens == lens).all()
                # every piece that had a pair to evaluate was one border call on the path set
                after = ctx.pairs_paths_taken()
                assert after[path] - taken[path] == len(PIECES) - 2, (taken, after)
                assert f32(ctx.collection_stat(col.h)[1]) == f32(thr)


# ----------------------------------------------------------------------------
# B. removal
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def survivor_reference(k):
    """The oracle's all-pairs list of the 508 rows that survive REMOVED, with its f64 ANI."""
    sk, lens = sweep_rows()
    keep = np.setdiff1d(np.arange(len(lens)), REMOVED)
    assert len(REMOVED) == 92 and len(keep) == 508
    q = quads(oracle.pairs(sk[keep], lens[keep].astype(np.int32), f32(0.0), k=k))
    assert len(q) == 508 * 507 // 2 == 128778
    ani = pair_ani(q, k)
    for a in (keep, q, ani):
        a.setflags(write=False)
    return keep, q, ani


def expected_new_index(n, removed):
    keep = np.ones(n, bool)
    keep[removed] = False
    out = np.full(n, NONE, np.uint32)
    out[keep] = np.arange(int(keep.sum()), dtype=np.uint32)
    return out


@pytest.mark.parametrize("k", [21, 2])
@pytest.mark.parametrize("batch", [None, "1", "7", "64"])
def test_removal_equals_the_oracle_on_the_survivors(monkeypatch, batch, k):
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(k)
    keep, sq, sani = survivor_reference(k)
    if batch is None:
        monkeypatch.delenv("GALAHGPU_TEST_COLLECTION_BATCH", raising=False)
    else:
        monkeypatch.setenv("GALAHGPU_TEST_COLLECTION_BATCH", batch)
    order = np.random.default_rng(83).permutation(np.concatenate([REMOVED, REMOVED[:9]]))  # any order, repeats
    with ga.Context(k=k, sketch_size=SWEEP_S) as ctx:
        for thr in border_thresholds(v):
            before = int((ani >= np.float64(thr)).sum())
            passing = sani >= np.float64(thr)
            if k == 21 and thr in (f32(0.95), f32(0.0)):  # (the counts the design note records)
                assert (before, int(passing.sum())) == ((52171, 37353) if thr else (179700, 128778))
            with Handle(ctx, thr) as col:
                assert col.add_rows(sk, lens) == before
                new_index = col.remove(order)
                assert (new_index == expected_new_index(600, REMOVED)).all()
                assert_collection(col, sq[passing], sani[passing], "k=%d min_ani=%r batch=%s" % (k, thr, batch))
                rows, rlens = col.rows()
                assert (rows == sk[keep]).all() and (rlens == lens[keep]).all()
                info = col.info()
                assert info["n_rows"] == 508 and info["rows_moved"] == 508  # (row 0 is removed: every survivor moves)


def test_removal_edges():
    """Nothing, the last row alone (no row moves), the removed rows added back
    (the oracle on the permuted rows), every row, and an empty collection."""
    sk, lens = sweep_rows()
    thr = f32(0.95)
    q, ani, _ = sweep_reference(21)
    passing = ani >= np.float64(thr)
    keep, sq, sani = survivor_reference(21)
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx, Handle(ctx, thr) as col:
        col.add_rows(sk, lens)
        assert (col.remove([]) == np.arange(600)).all() and col.info()["rows_moved"] == 0
        assert_collection(col, q[passing], ani[passing], "nothing removed")
        new_index = col.remove([599])
        assert new_index[599] == NONE and (new_index[:599] == np.arange(599)).all()
        assert col.info()["rows_moved"] == 0 and col.info()["n_rows"] == 599
        last = passing & (q[:, 1] < 599)
        assert_collection(col, q[last], ani[last], "last row removed")
        col.remove(REMOVED[REMOVED < 599])
        assert_collection(col, sq[sani >= np.float64(thr)], sani[sani >= np.float64(thr)], "in two steps")
        # back again: the survivors, then the removed rows
        assert col.add_rows(sk[REMOVED], lens[REMOVED]) > 0
        perm = np.concatenate([keep, REMOVED])
        pq = quads(oracle.pairs(sk[perm], lens[perm].astype(np.int32), thr, k=21))
        assert len(pq) == int(passing.sum())
        assert_collection(col, pq, pair_ani(pq, 21), "removed rows added back")
        rows, rlens = col.rows()
        assert (rows == sk[perm]).all() and (rlens == lens[perm]).all()
        # every row
        assert (col.remove(np.arange(600)) == NONE).all()
        info = col.info()
        assert info["n_rows"] == 0 and info["n_pairs"] == 0 and info["rows_moved"] == 0
        assert len(col.pairs()[0]) == 0 and len(col.rows()[0]) == 0
        assert len(col.remove([])) == 0
        # and it goes on from empty
        assert col.add_rows(sk[:70], lens[:70]) == int((passing & (q[:, 1] < 70)).sum())
        first = passing & (q[:, 1] < 70)
        assert_collection(col, q[first], ani[first], "after removing all")


# ----------------------------------------------------------------------------
# C. a failed call leaves the collection as it was
# ----------------------------------------------------------------------------
def snapshot(col):
    return col.ctx.collection_stat(col.h), col.pairs(), col.rows()


def assert_same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all()


def test_failures_leave_the_state(golden, tmp_path):
    thr = ga.parse_percentage(90)
    paths = golden["paths"]
    with ga.Context(k=21, sketch_size=1000) as ctx, Handle(ctx, thr) as col:
        assert col.add_files(paths[:12]) > 0
        was = snapshot(col)
        assert was[0][0]["n_rows"] == 12
        with pytest.raises(ga.GalahGpuError) as e:
            col.remove([3, 12])
        assert e.value.status == INVALID
        assert_same(snapshot(col), was)
        for order in ([0] * 12, list(range(11)) + [12], list(range(1, 12)) + [1]):
            with pytest.raises(ga.GalahGpuError) as e:
                col.cluster(0.95, order=order)
            assert e.value.status == INVALID
        with pytest.raises(ga.GalahGpuError) as e:
            col.cluster(float("nan"))
        assert e.value.status == INVALID
        assert_same(snapshot(col), was)
        with pytest.raises(ga.GalahGpuError) as e:
            col.add_files([paths[12], str(tmp_path / "missing.fna"), paths[13]])
        assert e.value.status == IO
        assert_same(snapshot(col), was)
        with pytest.raises(ga.GalahGpuError) as e:
            col.add_rows(np.zeros((1, 1000), np.uint64), np.array([1001], np.uint32))
        assert e.value.status == INVALID
        assert_same(snapshot(col), was)
        # and it goes on
        col.add_files(paths[12:])
        q, ani = golden_table(golden, thr)
        assert_collection(col, q, ani.astype(np.float64), "after the failures")
    with ga.Context(k=21, sketch_size=1000) as ctx:
        with pytest.raises(ga.GalahGpuError) as e:
            ctx.collection_create(float("nan"))
        assert e.value.status == INVALID
        q, ani = golden_table(golden, thr)
        pairs = np.zeros(len(q), ga.PAIR_DTYPE)
        for x, f in enumerate(("i", "j", "common", "total")):
            pairs[f] = q[:, x]
        for bad in (pairs[::-1], np.concatenate([pairs[:1], pairs])):  # not ascending; a repeat
            with pytest.raises(ga.GalahGpuError) as e:
                ctx.collection_load(golden["sketches"], golden["lens"], bad, np.resize(ani, len(bad)), thr)
            assert e.value.status == INVALID
        with pytest.raises(ga.GalahGpuError) as e:  # j >= n
            ctx.collection_load(golden["sketches"][:5], golden["lens"][:5], pairs, ani, thr)
        assert e.value.status == INVALID


# ----------------------------------------------------------------------------
# D. cluster
# ----------------------------------------------------------------------------
def orders(n):
    return {"identity": None, "reversed": np.arange(n)[::-1].copy(), "shuffled": np.random.default_rng(89).permutation(n)}


def test_cluster_in_any_order():
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(21)
    inner = v[(v > 0) & (v < 1)]
    min_ani = f32(inner[len(inner) // 2])
    passing = ani >= np.float64(min_ani)
    eq, ea = q[passing], ani[passing].astype(np.float32)
    above = f32(inner[(3 * len(inner)) // 4])
    assert above > min_ani and (ea >= above).any() and not (ea >= above).all()
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx, Handle(ctx, min_ani) as col:
        col.add_rows(sk[:300], lens[:300])
        col.add_rows(sk[300:], lens[300:])
        for name, order in orders(600).items():
            pos = np.arange(600) if order is None else np.argsort(order)
            relabelled = np.stack([pos[eq[:, 0]], pos[eq[:, 1]]], axis=1)
            for T in (f32(0.0), np.nextafter(min_ani, f32(0)), min_ani, above, f32(1.0)):
                exp = ga.cluster_pairs_host(600, relabelled, ea, T)
                got = col.cluster(float(T), order=order)
                assert (got == exp).all(), (name, T)
            assert len(np.unique(exp)) > 1
        assert_collection(col, eq, ani[passing], "after clustering")


@pytest.mark.parametrize("cluster_ani", [0.95, 0.99])
def test_cluster_on_the_golden_genomes(golden, cluster_ani):
    thr = ga.parse_percentage(90)
    q, ani = golden_table(golden, thr)
    n = len(golden["paths"])
    with ga.Context(k=21, sketch_size=1000) as ctx, Handle(ctx, thr) as col:
        col.add_rows(golden["sketches"][:20], golden["lens"][:20])
        col.add_rows(golden["sketches"][20:], golden["lens"][20:])
        for name, order in orders(n).items():
            pos = np.arange(n) if order is None else np.argsort(order)
            relabelled = np.stack([pos[q[:, 0]], pos[q[:, 1]]], axis=1)
            exp = cluster_ref.cluster_ref(n, relabelled, ani, f32(cluster_ani))
            assert (col.cluster(float(f32(cluster_ani)), order=order) == exp).all(), name


# ----------------------------------------------------------------------------
# E. files
# ----------------------------------------------------------------------------
def test_files_through_the_collection_class(golden, tmp_path):
    thr = ga.parse_percentage(90)
    paths = golden["paths"]
    assert len(paths) == 27
    pre = ga.FinchPreclusterer(thr, sketch_cache_dir=str(tmp_path / "cache"))
    clu = ga.FinchClusterer(0.95)
    gone = [paths[0], paths[9], paths[10], paths[19], paths[26]]
    back = [paths[26], paths[0], paths[10]]
    final = [p for p in paths if p not in gone] + back
    with pre.collection(reserve=4) as col:
        assert len(col) == 0 and col.paths == [] and len(col.cache()) == 0
        col.add(paths[:10])
        col.add(paths[10:20])
        col.add(paths[20:])
        q, ani = golden_table(golden, thr)
        assert col.paths == paths and col.cache() == table_cache(q, ani)
        with pytest.raises(ValueError, match="already present"):
            col.add(paths[3:4])
        with pytest.raises(ValueError, match="not present"):
            col.remove([str(tmp_path / "never.fna")])
        with pytest.raises(RuntimeError, match="Failed to sketch genomes with finch"):
            col.add([str(tmp_path / "missing.fna")])
        assert col.paths == paths
        col.remove(gone)
        assert len(col) == 22
        col.add(back)
        assert col.paths == final and len(final) == 25 and col.info()["n_rows"] == 25
        assert col.cache() == ga.FinchPreclusterer(thr).distances(final)
        assert col.cluster(clu) == ga.cluster(final, ga.FinchPreclusterer(thr), clu)
        order = np.random.default_rng(97).permutation(25)
        assert col.cluster(clu, order=order) == ga.cluster([final[g] for g in order], ga.FinchPreclusterer(thr), clu)
        with pytest.raises(ValueError):
            col.cluster(clu, order=np.arange(24))
        state = col.state()
        assert state.paths == final and state.cache() == col.cache()
        state.save(tmp_path / "collection.npz")
    loaded = ga.PreclusterState.load(tmp_path / "collection.npz")
    with pytest.raises(ValueError):
        ga.Collection.from_state(loaded, ga.FinchPreclusterer(ga.parse_percentage(95)))
    with ga.Collection.from_state(loaded, pre) as col:
        assert col.paths == final and col.cache() == loaded.cache()
        again = col.state()
        assert (again.sketches == loaded.sketches).all() and (again.lens == loaded.lens).all()
        assert (quads(again.pairs) == quads(loaded.pairs)).all()
        assert (again.ani.view(np.uint32) == loaded.ani.view(np.uint32)).all()
        # it continues as the one it was saved from would
        col.remove(final[:2])
        col.add([paths[9], paths[19]])
        now = final[2:] + [paths[9], paths[19]]
        assert col.paths == now and col.cache() == ga.FinchPreclusterer(thr).distances(now)
        assert col.cluster(clu) == ga.cluster(now, ga.FinchPreclusterer(thr), clu)
    assert len(os.listdir(tmp_path / "cache")) >= 27


# ----------------------------------------------------------------------------
# F. composition and knobs
# ----------------------------------------------------------------------------
def test_view_composes_with_preclusters_device():
    torch = torch_dev()
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(21)
    thr = f32(0.95)
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx, Handle(ctx, thr) as col:
        col.add_rows(sk, lens)
        col.remove(REMOVED)
        n, m = col.info()["n_rows"], col.info()["n_pairs"]
        d_sk, d_lens, d_pairs, d_ani = col.view()
        assert d_sk and d_lens and d_pairs and d_ani
        d_members = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        ns = ctx.preclusters_device(n, d_pairs, m, d_members, d_offsets)
        members = d_members.cpu().numpy().view(np.uint32)
        offsets = d_offsets.cpu().numpy().view(np.uint32)[:ns + 1]
        got = [members[offsets[s]:offsets[s + 1]].tolist() for s in range(ns)]
        pairs, _ = col.pairs()
        assert got == ga.preclusters(n, pairs) and 1 <= ns <= n
        # the device rows are the rows: added to a second collection from where they lie
        with Handle(ctx, thr) as other:
            assert other.add_rows_device(d_sk, d_lens, n) == m
            a, b = col.pairs(), other.pairs()
            assert (quads(a[0]) == quads(b[0])).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all()
            assert (other.rows()[0] == col.rows()[0]).all()


@pytest.mark.parametrize("config", ["index", "gate", "index_no_range"])
def test_pair_kernel_knobs_give_the_same_collection(monkeypatch, config):
    sk, lens = sweep_rows()
    q, ani, _ = sweep_reference(21)
    keep, sq, sani = survivor_reference(21)
    thr = f32(0.95)
    set_config(monkeypatch, CONFIGS[config])
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx, Handle(ctx, thr) as col:
        before = ctx.pair_paths()
        for a, b in ((0, 300), (300, 536), (536, 600)):
            col.add_rows(sk[a:b], lens[a:b])
        passing = ani >= np.float64(thr)
        assert_collection(col, q[passing], ani[passing], config)
        after = ctx.pair_paths()
        key = "gate" if config == "gate" else "index"
        assert after[key] - before[key] == 3 and after["index_abandoned"] == before["index_abandoned"], (before, after)
        col.remove(REMOVED)
        assert_collection(col, sq[sani >= np.float64(thr)], sani[sani >= np.float64(thr)], config + " after removal")
