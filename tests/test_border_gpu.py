"""Adding genomes to a finished run on the GPU: the border
forms of the index kernels and of the gate kernel, the device and file entry
points, and cluster_update.  Needs an MI355X.

Expected values come from the CPU oracle, from numpy or from
tests/cluster_ref.py only.  Bar: (i, j, common, total) identical and in (i, j)
order; f32 ANI identical where it is returned.

A  sweep: n_old at tile edges and on both sides of the row-range rule, every
   kernel and index build, thresholds on achievable values, k = 21 and 2
B  pairs(first n_old) U pairs_border == all pairs, no repeat
C  runs of 20 and of 200 rows around n_old (kRowSortedRun = 32), a mixed run
D  2,299 partners of one row: the large map, the split passes, the overflow
E  n = 65535 / 65537 (16-bit and 32-bit member rows)
F  pairs_border_device: capacity, append, count restored after an abandoned index
G  update_files and FinchPreclusterer.update on the 27 golden genomes
H  cluster_update
"""
import functools
import os

import numpy as np
import pytest

import cluster_ref
import galah_amd as ga
import oracle
from test_gpu_parity import adversarial_sketches
from test_pair_edges import (PATH_KEYS, SENTINEL, assert_pairs, capacity_rows, check_capacity_contract,
                             f32_neighbours, pair_ani, path_delta, quads, ring_rows, shared_hash_reference,
                             sweep_reference, sweep_rows, torch_dev, SWEEP_S)

pytestmark = pytest.mark.gpu

f32 = np.float32
INDEX_KNOBS = ("GALAHGPU_PAIRS_KERNEL", "GALAHGPU_INDEX_BUCKETS", "GALAHGPU_INDEX_SPLIT", "GALAHGPU_INDEX_RANGE",
               "GALAHGPU_INDEX_MAX_SPLIT", "GALAHGPU_INDEX_COST")

# name -> environment; "auto" leaves the choice to the library
CONFIGS = {
    "index": {"GALAHGPU_PAIRS_KERNEL": "index"},
    "gate": {"GALAHGPU_PAIRS_KERNEL": "gate"},
    "auto": {},
    "index_full_sort": {"GALAHGPU_PAIRS_KERNEL": "index", "GALAHGPU_INDEX_BUCKETS": "0"},
    "index_no_split": {"GALAHGPU_PAIRS_KERNEL": "index", "GALAHGPU_INDEX_SPLIT": "0"},
    "index_no_range": {"GALAHGPU_PAIRS_KERNEL": "index", "GALAHGPU_INDEX_RANGE": "0"},
}


def set_config(monkeypatch, env):
    for name in INDEX_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def border_of(q, n_old):
    """The rows of q ([m, 4] in (i, j) order) with j >= n_old."""
    return q[q[:, 1] >= n_old]


# ----------------------------------------------------------------------------
# A. sweep
# ----------------------------------------------------------------------------
SWEEP_N_OLD = (0, 1, 63, 64, 65, 300, 536, 599, 600)


def border_thresholds(v):
    """0.0, one achievable ANI value strictly between 0 and 1 with its two f32
    neighbours, and 0.95."""
    inner = v[(v > 0) & (v < 1)]
    return [f32(0.0)] + f32_neighbours(inner[len(inner) // 2]) + [f32(0.95)]


@pytest.mark.parametrize("k", [21, 2])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_border_sweep(monkeypatch, config, k):
    """600 rows (test_pair_edges.sweep_rows), the new rows starting at both
    ends, next to the 64-row tile edges, at 300 (half the rows: the ordinary
    build) and at 536 (64 of 600 rows: the row-range build)."""
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(k)
    n = len(lens)
    set_config(monkeypatch, CONFIGS[config])
    with ga.Context(k=k, sketch_size=SWEEP_S) as ctx:
        for thr in border_thresholds(v):
            if thr == 0 and config not in ("gate", "auto"):
                continue  # (every pair passes at 0: the gate kernel's case)
            passing = q[ani >= np.float64(thr)]
            assert 0 < len(passing) and (thr == 0 or len(passing) < len(q))
            for n_old in SWEEP_N_OLD:
                before = ctx.pair_paths()
                got = ctx.pairs_border(sk, lens, n_old, thr)
                assert_pairs(got, border_of(passing, n_old), "%s k=%d min_ani=%r n_old=%d" % (config, k, thr, n_old))
                d = path_delta(ctx, before)
                if n_old == n:  # nothing to evaluate
                    assert len(got) == 0 and not any(d.values())
                elif config.startswith("index"):
                    assert d["index"] == 1 and d["gate"] == 0 and d["index_abandoned"] == 0, (thr, n_old, d)
                    assert d["index_full_sort"] == (1 if config == "index_full_sort" else 0), (thr, n_old, d)
                elif config == "gate" or thr == 0:
                    assert d["gate"] == 1 and d["index"] == 0, (thr, n_old, d)
                else:  # auto, 600 rows: the index
                    assert d["index"] == 1 and d["gate"] == 0, (thr, n_old, d)
        with pytest.raises(ga.GalahGpuError) as e:
            ctx.pairs_border(sk, lens, n + 1, f32(0.95))
        assert e.value.status == 1


# ----------------------------------------------------------------------------
# B. the identity
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def identity_rows():
    sk, lens = adversarial_sketches(np.random.default_rng(53), 700, 64)
    q = quads(oracle.pairs(sk, lens.astype(np.int32), f32(0.0)))
    assert len(q) == 700 * 699 // 2
    ani = pair_ani(q, 21)
    for a in (sk, lens, q, ani):
        a.setflags(write=False)
    return sk, lens, q, ani


@pytest.mark.parametrize("min_ani", [0.0, 0.9])
def test_old_pairs_and_border_are_all_pairs(monkeypatch, min_ani):
    """pairs(rows[:n_old]) and pairs_border(rows, n_old) together hold exactly
    the oracle's all-pairs rows, none twice (identical, prefix, empty and
    extreme-valued rows)."""
    sk, lens, q, ani = identity_rows()
    set_config(monkeypatch, {})
    exp = q[ani >= np.float64(f32(min_ani))]
    assert len(exp) > 1000
    with ga.Context(k=21, sketch_size=64) as ctx:
        for n_old in (100, 448, 699):
            old = quads(ctx.pairs(sk[:n_old], lens[:n_old], f32(min_ani)))
            border = quads(ctx.pairs_border(sk, lens, n_old, f32(min_ani)))
            assert (old[:, 1] < n_old).all() and (border[:, 1] >= n_old).all()
            both = np.concatenate([old, border])
            assert len(np.unique(both[:, :2], axis=0)) == len(both), n_old
            both = both[np.lexsort((both[:, 1], both[:, 0]))]
            assert both.shape == exp.shape and (both == exp).all(), n_old
            assert_pairs(ctx.pairs_border(sk, lens, n_old, f32(min_ani)), border_of(exp, n_old), n_old)


# ----------------------------------------------------------------------------
# C. runs on both sides of kRowSortedRun
# ----------------------------------------------------------------------------
RUN_N, RUN_S = 600, 8


@functools.lru_cache(maxsize=None)
def run_rows():
    """600 rows of 8 hashes of their own, then: hash A in 20 rows, hash B in
    200 rows (runs the bucketed build stores in row order, g <= 32, and in
    arrival order), and two hashes that differ in their low word only, in 5
    rows each (one run of equal sort keys for the full build: index_mixed_kernel).
    Every run holds rows 0 and n - 1 and rows on both sides of either n_old."""
    rng = np.random.default_rng(59)
    n, s = RUN_N, RUN_S
    sk = rng.integers(2**40, 2**62, (n, s), dtype=np.uint64)
    A, B = np.uint64(2**62 + 12345), np.uint64(2**62 + 2**40 + 7)
    M1 = np.uint64(2**62 + 2**50)
    M2 = M1 + np.uint64(1)

    def members(count):
        fixed = [0, n - 1, 10, 305, 550]  # (both ends, and a row in every part the two n_old cut)
        rest = np.setdiff1d(np.arange(1, n - 1), fixed)
        return np.concatenate([fixed, rng.choice(rest, count - len(fixed), replace=False)])

    groups = {A: members(20), B: members(200), M1: np.array([0, 150, 310, 570, n - 1]),
              M2: np.array([0, 7, 320, 590, n - 1])}
    for col, (h, rows) in enumerate(groups.items()):
        for n_old in RUN_N_OLD:
            assert (rows < n_old).sum() >= 2 and (rows >= n_old).sum() >= 2
        sk[rows, col] = h
    sk.sort(axis=1)
    assert (np.diff(sk, axis=1) > 0).all()
    assert int(sk.max()).bit_length() == 63  # (M1 and M2 share the top 32 of 63 significant bits)
    lens = np.full(n, s, np.uint32)
    sk.setflags(write=False)
    lens.setflags(write=False)
    return sk, lens


RUN_N_OLD = (300, 540)  # half the rows: the ordinary build; 60 of 600: the row-range build


@pytest.mark.parametrize("config", ["index", "index_full_sort", "index_no_split", "index_no_range", "gate"])
def test_runs_around_the_first_new_row(monkeypatch, config):
    sk, lens = run_rows()
    exp = {}
    for thr in (f32(0.5), f32(0.92)):  # one shared hash of 8 passes 0.5 (ANI 0.90), two pass 0.92 (0.934)
        q, passing = shared_hash_reference(sk, lens, thr)
        assert passing.all() if thr == f32(0.5) else (passing.any() and not passing.all())
        exp[thr] = q[passing]
    set_config(monkeypatch, CONFIGS[config])
    with ga.Context(k=21, sketch_size=RUN_S) as ctx:
        for thr, e in exp.items():
            for n_old in RUN_N_OLD:
                b = border_of(e, n_old)
                assert (b[:, 0] == 0).any() and (b[:, 1] == RUN_N - 1).any() and (b[:, 0] >= n_old).any()
                assert_pairs(ctx.pairs_border(sk, lens, n_old, thr), b, "%s min_ani=%s n_old=%d" % (config, thr, n_old))
        paths = ctx.pair_paths()
        if config == "gate":
            assert paths["gate"] == 4 and paths["index"] == 0
        else:
            assert paths["index"] == 4 and paths["gate"] == 0 and paths["index_abandoned"] == 0, paths


# ----------------------------------------------------------------------------
# D. the partner map
# ----------------------------------------------------------------------------
MAP_N, MAP_N_OLD = 2300, 2200


@functools.lru_cache(maxsize=None)
def map_rows():
    """2,300 rows of 8 hashes that all share one: the last rows have up to
    2,299 partners.  The border's expected rows from the oracle's merge of
    every (i, j >= 2,200)."""
    rng = np.random.default_rng(61)
    sk = rng.integers(2**40, 2**63, (MAP_N, 8), dtype=np.uint64)
    sk[:, 0] = np.uint64(2**50 + 99)
    sk.sort(axis=1)
    assert (np.diff(sk, axis=1) > 0).all()
    lens = np.full(MAP_N, 8, np.uint32)
    jj = np.repeat(np.arange(MAP_N_OLD, MAP_N, dtype=np.uint32), MAP_N)
    ii = np.tile(np.arange(MAP_N, dtype=np.uint32), MAP_N - MAP_N_OLD)
    keep = ii < jj
    ii, jj = ii[keep], jj[keep]
    c, t = oracle.pair_list(sk, lens.astype(np.int32), ii, jj)
    q = np.column_stack([ii, jj, c, t]).astype(np.uint32)
    q = q[np.lexsort((q[:, 1], q[:, 0]))]
    assert (q[:, 2] == 1).all()
    thr = f32(0.5)
    assert (pair_ani(q, 21) >= np.float64(thr)).all() and oracle.ani(0, 1) < np.float64(thr)
    sk.setflags(write=False)
    q.setflags(write=False)
    return sk, lens, thr, q


@pytest.mark.parametrize("max_split,index_range", [(None, None), (None, "0"), ("0", "0"), ("0", None)])
def test_border_row_with_thousands_of_partners(monkeypatch, max_split, index_range):
    """The last rows have more than 1,536 partners (the small map's fill
    limit).  The 100 new rows are under 40% of the rows, so by default the
    row-range build runs, reads the longest run (2,300) before the pairs
    kernel and chooses the large map, which holds them in one pass;
    with GALAHGPU_INDEX_RANGE=0 the ordinary build queues the pairs kernel
    with the small map, and the rows are redone in split passes.
    GALAHGPU_INDEX_MAX_SPLIT=0 forbids the split: the small map overflows, the
    index is abandoned and the gate kernel gives the same rows.  (With the
    large map 2,299 partners fit without a split, so that case stays on the
    index whatever GALAHGPU_INDEX_MAX_SPLIT says.)"""
    sk, lens, thr, q = map_rows()
    env = {}
    if max_split is not None:
        env["GALAHGPU_INDEX_MAX_SPLIT"] = max_split
    if index_range is not None:
        env["GALAHGPU_INDEX_RANGE"] = index_range
    set_config(monkeypatch, env)
    with ga.Context(k=21, sketch_size=8) as ctx:
        assert_pairs(ctx.pairs_border(sk, lens, MAP_N_OLD, thr), q, (max_split, index_range))
        paths = ctx.pair_paths()
        if max_split == "0" and index_range == "0":
            assert paths == {"index": 0, "index_abandoned": 1, "gate": 1, "other": 0, "index_full_sort": 0}
            assert ctx.fallbacks()["index_to_gate"] == 1
        else:
            assert paths == {"index": 1, "index_abandoned": 0, "gate": 0, "other": 0, "index_full_sort": 0}


# ----------------------------------------------------------------------------
# E. row width
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65535, 65537])
def test_border_at_the_16_bit_row_edge(monkeypatch, n):
    """The last 70 rows of test_pair_edges.ring_rows as the new ones: their
    partners are row 0, rows near n / 2 and each other; members are stored as
    16-bit rows at n = 65535 and as 32-bit rows at 65537."""
    sk, lens = ring_rows(n)
    n_old = n - 70
    exp = {}
    for thr in (f32(0.95), f32(0.5)):
        q, passing = shared_hash_reference(sk, lens, thr)
        exp[thr] = border_of(q[passing], n_old)
        assert len(exp[thr]) > 0 and (exp[thr][:, 0] == 0).any()
    assert len(exp[f32(0.5)]) > len(exp[f32(0.95)]) and (exp[f32(0.5)][:, 0] >= n_old).any()
    for config in ("index", "index_no_range", "gate"):
        set_config(monkeypatch, CONFIGS[config])
        with ga.Context(k=21, sketch_size=sk.shape[1]) as ctx:
            for thr, e in exp.items():
                assert_pairs(ctx.pairs_border(sk, lens, n_old, thr), e, "%s n=%d min_ani=%s" % (config, n, thr))
            paths = ctx.pair_paths()
            assert paths["gate" if config == "gate" else "index"] == 2 and paths["index_abandoned"] == 0, paths


# ----------------------------------------------------------------------------
# F. pairs_border_device
# ----------------------------------------------------------------------------
def border_device_into(torch, ctx, d_sk, d_lens, n, n_old, thr, n_true, out_cap, initial, null_out=False):
    """One pairs_border_device call into a sentinel-filled buffer larger than
    any result -> (count after the call, the whole buffer [entries, 4])."""
    entries = max(out_cap, 5) + n_true + 64
    d_out = torch.full((entries * 4,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), initial, dtype=torch.int64, device="cuda")
    ctx.pairs_border_device(d_sk, d_lens, n, n_old, thr, 0 if null_out else d_out, out_cap, d_cnt)
    torch.cuda.synchronize()
    return int(d_cnt.item()), d_out.cpu().numpy().view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("config", ["gate", "index"])
def test_border_device_capacity_and_append(monkeypatch, config):
    """The contract of pairs_device (include/galahgpu.h) for the border:
    capacities below, at and above the result, the count starting at 0 and at
    5, a null output with out_cap = 0; and the resident-matrix use: the rows in
    a tensor with spare rows after them."""
    torch = torch_dev()
    sk, lens, thr, all_true = capacity_rows()
    n, n_old = len(lens), 450
    true_set = {r for r in all_true if r[1] >= n_old}
    m = len(true_set)
    assert m >= 50
    spare = 40  # (never read: n names the rows in use)
    d_sk = torch.full((n + spare, sk.shape[1]), -1, dtype=torch.int64, device="cuda")
    d_sk[:n] = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.full((n + spare,), sk.shape[1], dtype=torch.int32, device="cuda")
    d_lens[:n] = torch.from_numpy(lens.view(np.int32)).cuda()
    set_config(monkeypatch, CONFIGS[config])
    with ga.Context(k=21, sketch_size=sk.shape[1]) as ctx:
        for out_cap in (0, 1, m // 2, m - 1, m, m + 5):
            for initial in (0, 5):
                what = (config, out_cap, initial)
                count, buf = border_device_into(torch, ctx, d_sk, d_lens, n, n_old, thr, m, out_cap, initial)
                check_capacity_contract(count, buf, true_set, out_cap, initial, what)
        for initial in (0, 5):
            count, buf = border_device_into(torch, ctx, d_sk, d_lens, n, n_old, thr, m, 0, initial, null_out=True)
            assert count == initial + m and (buf == SENTINEL).all(), (config, "null output", initial)
        paths = ctx.pair_paths()
        assert paths["index" if config == "index" else "gate"] == 14 and paths["index_abandoned"] == 0, paths
        # n_old == n: nothing is launched, the count stays; n_old > n is refused
        count, buf = border_device_into(torch, ctx, d_sk, d_lens, n, n, thr, m, m, 5)
        assert count == 5 and (buf == SENTINEL).all() and ctx.pair_paths() == paths
        with pytest.raises(ga.GalahGpuError) as e:
            border_device_into(torch, ctx, d_sk, d_lens, n, n + 1, thr, m, m, 0)
        assert e.value.status == 1


def test_border_device_abandoned_index_restores_count(monkeypatch):
    """The last row with 2,997 single-hash partners and
    GALAHGPU_INDEX_MAX_SPLIT=0: the two new rows before it emit, the last
    one's partners overflow the LDS map and the index is abandoned.  The count
    goes back to its value before the launch (5, not 0) and the gate kernel
    appends from there, inside the capacity."""
    torch = torch_dev()
    rng = np.random.default_rng(67)
    s, n = 1000, 3000
    n_old = n - 3
    base = np.unique(rng.integers(1, 2**62, 4 * s, dtype=np.uint64))[:s]
    sk = np.zeros((n, s), np.uint64)
    lens = np.zeros(n, np.uint32)
    sk[n - 1], lens[n - 1] = base, s
    for i in range(n - 1):
        v = np.unique(np.concatenate([[base[i % s]], rng.integers(2**62, 2**63, 40, dtype=np.uint64)]))
        sk[i, :len(v)] = v
        lens[i] = len(v)
    thr = f32(0.001)
    jj = np.repeat(np.arange(n_old, n, dtype=np.uint32), n)
    ii = np.tile(np.arange(n, dtype=np.uint32), n - n_old)
    keep = ii < jj
    ii, jj = ii[keep], jj[keep]
    c, t = oracle.pair_list(sk, lens.astype(np.int32), ii, jj)
    q = np.column_stack([ii, jj, c, t]).astype(np.uint32)
    q = q[pair_ani(q, 21) >= np.float64(thr)]
    true_set = set(map(tuple, q.tolist()))
    m = len(true_set)
    assert m == len(q) >= n - 1 and (q[:, 1] == n - 3).any() and (q[:, 1] == n - 2).any()
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    set_config(monkeypatch, {"GALAHGPU_PAIRS_KERNEL": "index", "GALAHGPU_INDEX_MAX_SPLIT": "0"})
    with ga.Context(k=21, sketch_size=s) as ctx:
        count, buf = border_device_into(torch, ctx, d_sk, d_lens, n, n_old, thr, m, m // 2, 5)
        check_capacity_contract(count, buf, true_set, m // 2, 5, "abandoned index")
        assert ctx.pair_paths() == {"index": 0, "index_abandoned": 1, "gate": 1, "other": 0, "index_full_sort": 0}


# ----------------------------------------------------------------------------
# G. files
# ----------------------------------------------------------------------------
SPLIT_OLD = 20


def golden_table(golden, thr):
    """The golden pair table's rows passing thr: ([m, 4] u32 in (i, j) order, f32 ANI)."""
    rows = [r for r in golden["pairs"] if oracle.ani(r[2], r[3]) >= np.float64(thr)]
    q = np.array([r[:4] for r in rows], dtype=np.uint32).reshape(-1, 4)
    return q, np.array([np.float32(oracle.ani(r[2], r[3])) for r in rows], dtype=np.float32)


def test_update_files_on_the_golden_genomes(golden, tmp_path):
    thr = ga.parse_percentage(90)
    q, ani = golden_table(golden, thr)
    new = q[:, 1] >= SPLIT_OLD
    assert 0 < new.sum() < len(q)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        for cache_dir in (None, str(tmp_path / "cache"), str(tmp_path / "cache")):  # (none, filling, served)
            sk, lens, pairs, got_ani = ctx.update_files(golden["sketches"][:SPLIT_OLD], golden["lens"][:SPLIT_OLD],
                                                        golden["paths"][SPLIT_OLD:], thr, cache_dir=cache_dir)
            assert (sk == golden["sketches"][SPLIT_OLD:]).all() and (lens == golden["lens"][SPLIT_OLD:]).all()
            assert_pairs(pairs, q[new], "update_files")
            assert got_ani.dtype == np.float32 and (got_ani.view(np.uint32) == ani[new].view(np.uint32)).all()
        assert len(os.listdir(tmp_path / "cache")) >= len(golden["paths"]) - SPLIT_OLD
        # no old rows: the whole run; no new files: nothing
        sk, lens, pairs, got_ani = ctx.update_files(golden["sketches"][:0], golden["lens"][:0], golden["paths"], thr)
        assert (sk == golden["sketches"]).all() and (lens == golden["lens"]).all()
        assert_pairs(pairs, q, "update_files from nothing")
        assert (got_ani.view(np.uint32) == ani.view(np.uint32)).all()
        sk, lens, pairs, got_ani = ctx.update_files(golden["sketches"], golden["lens"], [], thr)
        assert len(sk) == len(lens) == len(pairs) == len(got_ani) == 0


@functools.lru_cache(maxsize=None)
def golden_state(thr_bits):
    from conftest import golden_path, load_golden_sketches
    names, _, _ = load_golden_sketches()
    thr = np.array([thr_bits], np.uint32).view(np.float32)[0]
    return ga.FinchPreclusterer(thr).distances_state([golden_path(x) for x in names[:SPLIT_OLD]])


def table_cache(q, ani):
    cache = ga.SortedPairGenomeDistanceCache()
    for r, a in zip(q, ani):
        cache.insert((int(r[0]), int(r[1])), np.float32(a))
    return cache


def test_preclusterer_update_on_the_golden_genomes(golden, tmp_path):
    thr = ga.parse_percentage(90)
    q, ani = golden_table(golden, thr)
    old = golden_state(int(thr.view(np.uint32)))
    assert old.paths == golden["paths"][:SPLIT_OLD] and (old.k, old.s, old.seed) == (21, 1000, 0)
    assert (old.sketches == golden["sketches"][:SPLIT_OLD]).all() and (old.lens == golden["lens"][:SPLIT_OLD]).all()
    was = q[:, 1] < SPLIT_OLD
    assert old.cache() == table_cache(q[was], ani[was])
    old.save(tmp_path / "run.npz")
    pre = ga.FinchPreclusterer(thr)
    new = pre.update(ga.PreclusterState.load(tmp_path / "run.npz"), golden["paths"][SPLIT_OLD:])
    assert new.paths == golden["paths"]
    assert (new.sketches == golden["sketches"]).all() and (new.lens == golden["lens"]).all()
    assert_pairs(new.pairs, q, "state after update")
    assert (new.ani.view(np.uint32) == ani.view(np.uint32)).all()
    assert new.cache() == table_cache(q, ani) and len(new.cache()) == len(q)
    with pytest.raises(ValueError):
        ga.FinchPreclusterer(ga.parse_percentage(95)).update(old, golden["paths"][SPLIT_OLD:])
    with pytest.raises(ValueError, match="already present"):
        pre.update(new, golden["paths"][3:4])


# ----------------------------------------------------------------------------
# H. cluster_update
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("cluster_ani", [0.95, 0.99])
@pytest.mark.parametrize("order_kind", ["default", "interleaved"])
def test_cluster_update_on_the_golden_genomes(golden, order_kind, cluster_ani):
    """20 old and 7 new genomes: the clusters are those of the reference's two
    loops (tests/cluster_ref.py) over the golden pair table relabelled into the
    order the genomes are clustered in."""
    thr = ga.parse_percentage(90)
    q, ani = golden_table(golden, thr)
    n = len(golden["paths"])
    order = np.arange(n)
    if order_kind == "interleaved":  # a random order with a new genome ahead of every old one
        order = np.random.default_rng(71).permutation(n)
        p = int(np.flatnonzero(order == SPLIT_OLD + 2)[0])
        order[0], order[p] = order[p], order[0]
        assert order[0] >= SPLIT_OLD and (np.diff(order) < 0).any()
    pos = np.argsort(order)  # genome -> position
    relabelled = np.stack([pos[q[:, 0]], pos[q[:, 1]]], axis=1)
    exp = cluster_ref.clusters_ref(cluster_ref.cluster_ref(n, relabelled, ani, f32(cluster_ani)))
    assert 1 < len(exp) <= n
    old = golden_state(int(thr.view(np.uint32)))
    clusters, new = ga.cluster_update(old, golden["paths"][SPLIT_OLD:], ga.FinchPreclusterer(thr),
                                      ga.FinchClusterer(cluster_ani), order=None if order_kind == "default" else order)
    assert clusters == exp
    assert new.paths == golden["paths"]
    assert_pairs(new.pairs, q, "state after cluster_update")
    with pytest.raises(ValueError):
        ga.cluster_update(old, golden["paths"][SPLIT_OLD:], ga.FinchPreclusterer(thr), ga.FinchClusterer(cluster_ani),
                          order=np.arange(n - 1))
