"""Edges of the pair path (K2: pairs_gate.hip, pairs_index.hip, the
cmin / sufmin tables and the index plumbing of api.cpp) against the CPU
oracle or plain numpy, never against another GPU kernel.  Needs an MI355X.

Bar: (i, j, common, total) identical and in (i, j) order; ANI f32 identical
where it is returned.

A  thresholds on and next to achievable ANI values, every pair kernel, k != 21
B  gg_pairs_device: output capacity, append at a non-zero count, null output
C  the index -> gate cost fallback (GALAHGPU_INDEX_COST) at its three host sites
D  n = 65535 / 65536 / 65537 (16-bit row ids of the bucketed index)
E  4095 / 4096 / 4097 pairs (host sort / device sort of the result)
F  s = kMaxSketch = 12000 (the gate kernel's 8-bit per-lane counters)
G  genomes without a valid k-mer through the fused file call
"""
import functools
import shutil

import numpy as np
import pytest

import galah_amd as ga
import oracle
from conftest import xcheck_module
from test_gpu_parity import adversarial_sketches, random_sketch_set

pytestmark = pytest.mark.gpu

f32 = np.float32
PATH_KEYS = ("index", "index_abandoned", "gate", "other", "index_full_sort")


def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


def quads(p):
    """[m, 4] u32 (i, j, common, total) of a pair array, in its order."""
    return np.stack([p["i"], p["j"], p["common"], p["total"]], axis=1).astype(np.uint32).reshape(-1, 4)


def assert_pairs(got, exp, what):
    """got (a pair array) holds exactly the rows of exp ([m, 4]) in exp's order."""
    g = quads(got)
    if g.shape == exp.shape and (g == exp).all():
        return
    gs, es = set(map(tuple, g.tolist())), set(map(tuple, exp.tolist()))
    raise AssertionError("%s: %d pairs, expected %d; missing %s; unexpected %s; %s" % (
        what, len(g), len(exp), sorted(es - gs)[:5], sorted(gs - es)[:5],
        "same set, other order or repeats" if gs == es else "sets differ"))


def pair_ani(q, k):
    """The oracle's f64 ANI of every row of q ([m, 4]), one call per distinct (common, total)."""
    u, inv = np.unique(q[:, 2:], axis=0, return_inverse=True)
    return oracle.ani_array(u[:, 0], u[:, 1], k)[inv.reshape(-1)]


def module_for(kern):
    # (table, merge: the cross-check kernels of the test build)
    return xcheck_module() if kern in ("table", "merge") else ga


def path_delta(ctx, before):
    after = ctx.pair_paths()
    return {key: after[key] - before[key] for key in PATH_KEYS}


# ----------------------------------------------------------------------------
# A. threshold boundaries
# ----------------------------------------------------------------------------
SWEEP_N, SWEEP_S = 600, 32


@functools.lru_cache(maxsize=None)
def sweep_rows():
    """600 rows of at most 32 hashes drawn from nested prefixes of one pool of
    ~160 values: ~1,000 distinct (common, total) with totals 1..62."""
    rng = np.random.default_rng(7)
    n, s = SWEEP_N, SWEEP_S
    U = np.unique(rng.integers(1, 2**63, 5 * s, dtype=np.uint64))
    sk = np.zeros((n, s), np.uint64)
    lens = np.zeros(n, np.uint32)
    for i in range(n):
        m = s if i % 4 < 2 else int(rng.integers(1, s + 1))
        width = int(rng.integers(m, len(U) + 1))
        sk[i, :m] = np.sort(rng.choice(U[:width], m, replace=False))
        lens[i] = m
    sk.setflags(write=False)
    lens.setflags(write=False)
    return sk, lens


def f32_neighbours(x):
    x = f32(x)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def sweep_thresholds(v, n_values):
    """~n_values of the sorted distinct ANI values v evenly spaced, the
    smallest non-zero one and the largest below 1, each as f32 with its two
    f32 neighbours, and the fixed set."""
    idx = np.unique(np.round(np.linspace(0, len(v) - 1, n_values)).astype(np.int64))
    picked = list(v[idx]) + [v[v > 0][0], v[v < 1][-1]]
    thrs = [t for x in picked for t in f32_neighbours(x)]
    thrs += [f32(0.0), np.nextafter(f32(0), f32(1)), f32(0.9), f32(0.95), f32(0.99), f32(1.0),
             np.nextafter(f32(1), f32(2))]
    seen = {}
    for t in thrs:
        seen.setdefault(int(f32(t).view(np.uint32)), f32(t))
    return list(seen.values())


@functools.lru_cache(maxsize=None)
def sweep_reference(k):
    """Every pair's (i, j, common, total) and f64 ANI at k, from the oracle,
    with the coverage this test relies on asserted."""
    sk, lens = sweep_rows()
    n = len(lens)
    q = quads(oracle.pairs(sk, lens.astype(np.int32), f32(0.0), k=k))
    assert len(q) == n * (n - 1) // 2
    ani = pair_ani(q, k)
    v = np.unique(ani)
    as32 = v.astype(np.float32).astype(np.float64)
    assert len(np.unique(q[:, 2:], axis=0)) >= 800
    assert int((as32 > v).sum()) >= 200 and int((as32 < v).sum()) >= 200
    assert (ani == 1.0).any() and (q[:, 2] == 0).any()
    if k == 2:  # mash distance clamped at 1: ANI exactly 0 with common > 0
        assert int(((ani == 0.0) & (q[:, 2] > 0)).sum()) >= 1000
    # the filter of the all-pairs list is the oracle's own answer at a
    # threshold: on a value that rounds up in f32, on one that rounds down,
    # and at the smallest subnormal
    up, down = v[as32 > v], v[(as32 < v) & (v < 1)]
    for thr in (f32(up[len(up) // 2]), f32(down[len(down) // 2]), np.nextafter(f32(0), f32(1))):
        o = quads(oracle.pairs(sk, lens.astype(np.int32), thr, k=k))
        assert (o == q[ani >= np.float64(thr)]).all() and len(o) == int((ani >= np.float64(thr)).sum())
    assert not (ani[q[:, 2] > 0] >= np.float64(f32(up[len(up) // 2]))).all()
    for a in (q, ani, v):
        a.setflags(write=False)
    return q, ani, v


# gate and index at every k; auto and the cross-check kernels at k = 21
SWEEP_CASES = [(kern, k) for kern in ("gate", "index") for k in (21, 16, 32, 2)] + \
              [(kern, 21) for kern in ("auto", "table", "merge")]


@pytest.mark.parametrize("kern,k", SWEEP_CASES)
def test_threshold_boundaries(monkeypatch, kern, k):
    """A pair passes when ani_f64(common, total, k) >= (double)(float)min_ani;
    the kernels compare common with cmin[total] (api.cpp build_cmin, a binary
    search) and prefilter with sufmin.  Thresholds on achievable ANI values
    narrowed to f32 (about half round up, so the pair itself fails; half
    round down, so it passes) and on their f32 neighbours, at k = 21, 16, 32
    and at k = 2, where the mash distance clamps at 1 for pairs with
    common > 0 (ANI exactly 0: they fail at the smallest subnormal)."""
    sk, lens = sweep_rows()
    q, ani, v = sweep_reference(k)
    thrs = sweep_thresholds(v, 64)
    as32 = v.astype(np.float32).astype(np.float64)
    # thresholds on values that round up and on values that round down
    bits = {int(t.view(np.uint32)) for t in thrs}
    on = np.array([int(f32(x).view(np.uint32)) in bits for x in v])
    assert int((on & (as32 > v)).sum()) >= 10 and int((on & (as32 < v)).sum()) >= 10
    monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", kern)
    with module_for(kern).Context(k=k, sketch_size=SWEEP_S) as ctx:
        for thr in thrs:
            before = ctx.pair_paths()
            got = ctx.pairs(sk, lens, thr)
            assert_pairs(got, q[ani >= np.float64(thr)], "%s k=%d min_ani=%r" % (kern, k, thr))
            if kern == "index":
                # any threshold > 0, the smallest subnormal included, leaves no
                # pass without a shared hash (ANI(0, t) is exactly 0): the
                # index runs; at <= 0 every pair passes and the gate kernel runs
                d = path_delta(ctx, before)
                if thr > 0:
                    assert d == {"index": 1, "index_abandoned": 0, "gate": 0, "other": 0, "index_full_sort": 0}, thr
                else:
                    assert d == {"index": 0, "index_abandoned": 0, "gate": 1, "other": 0, "index_full_sort": 0}, thr


# ----------------------------------------------------------------------------
# B. gg_pairs_device: capacity and append
# ----------------------------------------------------------------------------
SENTINEL = np.uint32(0xFFFFFFFF)


def pairs_device_into(torch, ctx, d_sk, d_lens, n, thr, n_true, out_cap, initial, null_out=False):
    """One full-range gg_pairs_device call into a sentinel-filled buffer larger
    than any result -> (count after the call, the whole buffer [entries, 4])."""
    entries = max(out_cap, 5) + n_true + 64
    d_out = torch.full((entries * 4,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), initial, dtype=torch.int64, device="cuda")
    ctx.pairs_device(d_sk, d_lens, n, 0, ga.pair_tiles(n), thr, 0 if null_out else d_out, out_cap, d_cnt)
    torch.cuda.synchronize()
    return int(d_cnt.item()), d_out.cpu().numpy().view(np.uint32).reshape(-1, 4)


def check_capacity_contract(count, buf, true_set, out_cap, initial, what):
    """include/galahgpu.h: *d_count incremented by the number found, entries
    past out_cap dropped (nothing written there), earlier entries kept."""
    assert count == initial + len(true_set), what
    assert (buf[out_cap:] == SENTINEL).all(), what
    assert (buf[:initial] == SENTINEL).all(), what
    got = [tuple(r) for r in buf[initial:min(out_cap, count)].tolist()]
    assert len(set(got)) == len(got) and set(got) <= true_set, what
    if out_cap >= initial + len(true_set):
        assert set(got) == true_set, what


@functools.lru_cache(maxsize=None)
def capacity_rows():
    sk, lens = random_sketch_set(np.random.default_rng(9), 600, 64, 5)
    thr = f32(0.9)
    true = quads(oracle.pairs(sk, lens.astype(np.int32), thr))
    true_set = set(map(tuple, true.tolist()))
    assert len(true_set) == len(true) >= 200
    return sk, lens, thr, true_set


@pytest.mark.parametrize("kern", ["gate", "index", "table", "merge"])
def test_pairs_device_capacity_and_append(monkeypatch, kern):
    """Output capacities below, at and above the result with *d_count starting
    at 0 and at 5 (the `slot < out_cap` guard of each kernel, the append), and
    a null output with out_cap = 0 (counting only)."""
    torch = torch_dev()
    sk, lens, thr, true_set = capacity_rows()
    n, m = len(lens), len(true_set)
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", kern)
    with module_for(kern).Context(k=21, sketch_size=64) as ctx:
        for out_cap in (0, 1, m // 2, m - 1, m, m + 5):
            for initial in (0, 5):
                what = (kern, out_cap, initial)
                count, buf = pairs_device_into(torch, ctx, d_sk, d_lens, n, thr, m, out_cap, initial)
                check_capacity_contract(count, buf, true_set, out_cap, initial, what)
        for initial in (0, 5):
            count, buf = pairs_device_into(torch, ctx, d_sk, d_lens, n, thr, m, 0, initial, null_out=True)
            assert count == initial + m and (buf == SENTINEL).all(), (kern, "null output", initial)
        paths = ctx.pair_paths()
        if kern == "index":
            assert paths["index"] == 14 and paths["gate"] == 0 and paths["index_abandoned"] == 0, paths
        elif kern == "gate":
            assert paths["gate"] == 14 and paths["index"] == 0, paths
        else:
            assert paths["other"] == 14, paths


def test_pairs_device_abandoned_index_restores_count(monkeypatch):
    """Row 0 with 2,999 single-hash partners and GALAHGPU_INDEX_MAX_SPLIT=0:
    the index launch emits, then is abandoned (a row's partners overflow the
    LDS map).  The count goes back to its value before the launch (5, not 0)
    and the gate kernel appends from there, inside the capacity."""
    torch = torch_dev()
    rng = np.random.default_rng(29)
    s, n = 1000, 3000
    base = np.unique(rng.integers(1, 2**62, 4 * s, dtype=np.uint64))[:s]
    sk = np.zeros((n, s), np.uint64)
    lens = np.zeros(n, np.uint32)
    sk[0], lens[0] = base, s
    for i in range(1, n):
        v = np.unique(np.concatenate([[base[i % s]], rng.integers(2**62, 2**63, 40, dtype=np.uint64)]))
        sk[i, :len(v)] = v
        lens[i] = len(v)
    thr = f32(0.001)
    true = quads(oracle.pairs(sk, lens.astype(np.int32), thr))
    true_set = set(map(tuple, true.tolist()))
    m = len(true_set)
    assert m == len(true) >= n - 1
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", "index")
    monkeypatch.setenv("GALAHGPU_INDEX_MAX_SPLIT", "0")
    with ga.Context(k=21, sketch_size=s) as ctx:
        count, buf = pairs_device_into(torch, ctx, d_sk, d_lens, n, thr, m, m // 2, 5)
        check_capacity_contract(count, buf, true_set, m // 2, 5, "abandoned index")
        assert ctx.pair_paths() == {"index": 0, "index_abandoned": 1, "gate": 1, "other": 0, "index_full_sort": 0}


# ----------------------------------------------------------------------------
# C. the index -> gate cost fallback
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_rows():
    sk, lens = random_sketch_set(np.random.default_rng(23), 701, 1000, 9)
    exp = quads(oracle.pairs(sk, lens.astype(np.int32), f32(0.9)))
    assert len(exp) > 0
    exp.setflags(write=False)
    return sk, lens, exp


def tile_rows_of(n, tb, te):
    """[r0, r1): the rows of the tile rows that hold tiles [tb, te) (tiles
    numbered tile row by tile row, tile row I holding columns I..nb-1)."""
    nb = (n + ga.GG_PAIR_TILE - 1) // ga.GG_PAIR_TILE
    t, rows = 0, []
    for I in range(nb):
        first, last = t, t + (nb - I)
        t = last
        if max(first, tb) < min(last, te):
            rows.append(I)
    return rows[0] * ga.GG_PAIR_TILE, min(n, (rows[-1] + 1) * ga.GG_PAIR_TILE)


@pytest.mark.parametrize("site", ["bucketed", "full_sort", "row_range"])
def test_index_cost_fallback(monkeypatch, site):
    """GALAHGPU_INDEX_COST (off by default) under the default kernel choice:
    at 1e-9 any shared hash outweighs the gate kernel, so every call builds
    the index, abandons it before emitting and runs the gate kernel -- from
    the bucketed full-range build (the pairs kernel already queued: its own
    early exit), from the full sort (GALAHGPU_INDEX_BUCKETS=0) and from the
    row-range bucketed build of a multi-device part; at 1e9 the same calls
    take the index."""
    torch = torch_dev()
    sk, lens, exp = cost_rows()
    n = len(lens)
    thr = f32(0.9)
    monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", "auto")
    if site == "full_sort":
        monkeypatch.setenv("GALAHGPU_INDEX_BUCKETS", "0")
    parts = 7
    ranges = [ga.pair_partition(n, parts, p) for p in range(parts)]
    if site == "row_range":
        # every part holds tiles; at least one spans <= 40% of the rows (the
        # row-range Bloom build of api.cpp pairs_index), at least one more
        assert ranges[0][0] == 0 and ranges[-1][1] == ga.pair_tiles(n)
        assert all(b < e for b, e in ranges) and all(ranges[p][1] == ranges[p + 1][0] for p in range(parts - 1))
        spans = [r1 - r0 for r0, r1 in (tile_rows_of(n, b, e) for b, e in ranges)]
        assert any(5 * x <= 2 * n for x in spans), spans
        d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
        d_lens = torch.from_numpy(lens.view(np.int32)).cuda()

    def run(ctx):
        if site != "row_range":
            assert_pairs(ctx.pairs(sk, lens, thr), exp, site)
            return 1
        got = []
        cap = len(exp) + 64
        for b, e in ranges:
            d_out = torch.zeros(cap * 4, dtype=torch.int32, device="cuda")
            d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx.pairs_device(d_sk, d_lens, n, b, e, thr, d_out, cap, d_cnt)
            torch.cuda.synchronize()
            c = int(d_cnt.item())
            assert c <= cap
            got.append(d_out[:c * 4].cpu().numpy().view(np.uint32).reshape(-1, 4))
        got = np.concatenate(got)
        got = got[np.lexsort((got[:, 1], got[:, 0]))]
        assert got.shape == exp.shape and (got == exp).all(), site
        return parts

    monkeypatch.setenv("GALAHGPU_INDEX_COST", "1e-9")
    with ga.Context(k=21, sketch_size=1000) as ctx:
        calls = run(ctx)
        assert ctx.pair_paths() == {"index": 0, "index_abandoned": calls, "gate": calls, "other": 0,
                                    "index_full_sort": int(site == "full_sort")}
        assert ctx.fallbacks()["index_to_gate"] == calls
        assert "index->gate by cost %d;" % calls in ctx.info_line()
    # the knob is what switches
    monkeypatch.setenv("GALAHGPU_INDEX_COST", "1e9")
    with ga.Context(k=21, sketch_size=1000) as ctx:
        calls = run(ctx)
        assert ctx.pair_paths() == {"index": calls, "index_abandoned": 0, "gate": 0, "other": 0,
                                    "index_full_sort": int(site == "full_sort")}
        assert ctx.fallbacks()["index_to_gate"] == 0 and "by cost" not in ctx.info_line()


# ----------------------------------------------------------------------------
# D. n at the 16-bit row edge
# ----------------------------------------------------------------------------
def ring_rows(n, s=8):
    """n rows of 8 hashes: one shared with each ring neighbour (r +- 1 mod n),
    one with row r + n // 2, and rows 0, 65534, 65535, 65536 and n - 1 (those
    below n) sharing five more."""
    rng = np.random.default_rng(n)
    draw = lambda *shape: rng.integers(2**40, 2**63, shape, dtype=np.uint64)
    sk = draw(n, s)
    link = draw(n)
    sk[:, 0] = link
    sk[:, 1] = np.roll(link, 1)
    sk[:, 2] = draw(n // 2)[np.arange(n) % (n // 2)]
    near = sorted({r for r in (0, 65534, 65535, 65536, n - 1) if r < n})
    sk[near, 3:] = draw(s - 3)
    sk.sort(axis=1)
    assert (np.diff(sk, axis=1) > 0).all()
    return sk, np.full(n, s, np.uint32)


def shared_hash_reference(sk, lens, thr, k=21):
    """The passing pairs [m, 4] in (i, j) order without the all-pairs loop:
    only rows that share a hash can pass (asserted), so the candidates are
    the row pairs inside each group of equal hash values."""
    n, s = sk.shape
    assert all(oracle.ani(0, t, k) < np.float64(thr) for t in range(1, 2 * s + 1))
    assert (lens == s).all()
    vals = sk.reshape(-1)
    rows = np.repeat(np.arange(n, dtype=np.uint32), s)
    order = np.argsort(vals, kind="stable")
    sv, sr = vals[order], rows[order]
    cand, d = [], 1
    while True:  # equal values are adjacent: members d apart inside one group
        eq = sv[d:] == sv[:-d]
        if not eq.any():
            break
        a, b = sr[:-d][eq], sr[d:][eq]
        cand.append(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1))
        d += 1
    cand = np.unique(np.concatenate(cand), axis=0)  # (i, j) order
    assert (cand[:, 0] < cand[:, 1]).all()
    c, t = oracle.pair_list(sk, lens.astype(np.int32), cand[:, 0], cand[:, 1])
    q = np.column_stack([cand, c, t]).astype(np.uint32)
    passing = pair_ani(q, k) >= np.float64(thr)
    return q, passing


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_rows_at_the_16_bit_edge(monkeypatch, n):
    """The bucketed index stores its members as 16-bit rows up to n = 65536
    (pairs_index.hip index_ents16) and as 32-bit rows from 65537: the last
    rows on both sides pair with row 0 and with each other.  At min_ani 0.5
    all ~10^5 candidate pairs pass and go through the device sort of the
    result."""
    sk, lens = ring_rows(n)
    # at 0.95 only the near-identical rows pass (the candidates split); at 0.5
    # one shared hash of 8 is enough, so every candidate passes
    exp = {}
    for thr in (f32(0.95), f32(0.5)):
        q, passing = shared_hash_reference(sk, lens, thr)
        exp[thr] = q[passing]
        if thr == f32(0.95):
            assert passing.any() and (~passing).any()
        else:
            assert passing.all() and len(q) > n
        for r in range(65534, n):
            assert (exp[thr][:, :2] == r).any(), r
    for kern in ("index", "gate"):
        monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", kern)
        with ga.Context(k=21, sketch_size=sk.shape[1]) as ctx:
            for thr in exp:
                assert_pairs(ctx.pairs(sk, lens, thr), exp[thr], "%s n=%d min_ani=%s" % (kern, n, thr))
            paths = ctx.pair_paths()
            if kern == "index":
                assert paths == {"index": 2, "index_abandoned": 0, "gate": 0, "other": 0, "index_full_sort": 0}
            else:
                assert paths["gate"] == 2 and paths["index"] == 0


# ----------------------------------------------------------------------------
# E. the host sort / device sort switch
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("count", [4095, 4096, 4097])
def test_result_sort_switch(monkeypatch, count):
    """pairs_range_to_host sorts fewer than kDeviceSortPairs = 4096 pairs on
    the host and 4096 or more on the device: 91 identical rows (4,095 pairs at
    min_ani 1.0) and 0, 1 or 2 further identical pairs of rows, their members
    apart, rows that match nothing between them."""
    rng = np.random.default_rng(count)
    s = 16
    def draw():
        v = np.unique(rng.integers(1, 2**62, s, dtype=np.uint64))
        assert len(v) == s
        return v

    cluster = draw()
    rows = []
    for _ in range(91):
        rows += [cluster, draw()]
    for _ in range(count - 4095):
        twin = draw()
        rows += [twin, draw(), draw(), twin]
    sk = np.stack(rows)
    lens = np.full(len(rows), s, np.uint32)
    exp = quads(oracle.pairs(sk, lens.astype(np.int32), f32(1.0)))
    assert len(exp) == count
    for kern in ("gate", "index"):
        monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", kern)
        with ga.Context(k=21, sketch_size=s) as ctx:
            assert_pairs(ctx.pairs(sk, lens, f32(1.0)), exp, "%s %d pairs" % (kern, count))
            assert ctx.pair_paths()["index" if kern == "index" else "gate"] == 1


# ----------------------------------------------------------------------------
# F. the largest sketch size
# ----------------------------------------------------------------------------
MAX_SKETCH = 12000  # gg_internal.hpp kMaxSketch


@functools.lru_cache(maxsize=None)
def max_sketch_rows():
    sk, lens = adversarial_sketches(np.random.default_rng(MAX_SKETCH), 24, MAX_SKETCH)
    assert lens.max() == MAX_SKETCH and lens.min() == 0
    return sk, lens


@pytest.mark.parametrize("min_ani", [0.0, 0.9])
def test_largest_sketch_size(monkeypatch, min_ani):
    """s = 12000: 188 hashes per lane, the most the gate kernel's 8-bit
    per-lane hit counters are sized for (identical rows hit in every slot)."""
    sk, lens = max_sketch_rows()
    exp = quads(oracle.pairs(sk, lens.astype(np.int32), f32(min_ani)))
    assert len(exp) > 0 and (exp[:, 2] == MAX_SKETCH).any()
    for kern in ("gate", "index", "merge"):
        monkeypatch.setenv("GALAHGPU_PAIRS_KERNEL", kern)
        with module_for(kern).Context(k=21, sketch_size=MAX_SKETCH) as ctx:
            assert_pairs(ctx.pairs(sk, lens, f32(min_ani)), exp, "%s min_ani=%s" % (kern, min_ani))


def test_sketch_size_past_the_largest_is_refused():
    with pytest.raises(ga.GalahGpuError) as e:
        ga.Context(k=21, sketch_size=MAX_SKETCH + 1)
    assert e.value.status == 1  # GG_ERR_INVALID_ARG
    ga.Context(k=21, sketch_size=MAX_SKETCH).close()


# ----------------------------------------------------------------------------
# G. genomes without a valid k-mer
# ----------------------------------------------------------------------------
def test_genomes_without_kmers_through_the_fused_call(gpu_ctx, golden, tmp_path):
    """All-N, shorter than k and record-less genomes sketch to nothing: next
    to real genomes gg_precluster_files gives the oracle's pairs and f32 ANI.
    Two empty sketches compare as (common 0, total 0): ANI 0.0, which passes
    min_ani 0.0 and nothing above."""
    paths = []
    for x, name in enumerate(("set1/1mbp.fna", "set1/500kb.fna", "set1_name_clash/500kb.fna")):
        p = tmp_path / ("g%d.fna.gz" % x)
        shutil.copyfile(golden["paths"][golden["names"].index(name)], p)
        paths.append(str(p))
    empties = {"all_n.fna": b">n\n" + b"\n".join([b"N" * 100] * 50) + b"\n",
               "short.fna": b">s\nACGTACGTACGTACGTACGT\n",
               "header_only.fna": b">h\n\n",
               "all_n_again.fna": b">n\n" + b"\n".join([b"N" * 100] * 50) + b"\n"}
    for name, text in empties.items():
        (tmp_path / name).write_bytes(text)
    paths = [paths[0], str(tmp_path / "all_n.fna"), paths[1], str(tmp_path / "short.fna"),
             str(tmp_path / "header_only.fna"), paths[2], str(tmp_path / "all_n_again.fna")]
    empty = (1, 3, 4, 6)
    sk, lens = oracle.sketch_files(paths)
    assert [int(lens[g]) for g in empty] == [0, 0, 0, 0] and all(lens[g] == 1000 for g in (0, 2, 5))
    for thr in (f32(0.0), ga.parse_percentage(90)):
        o = oracle.pairs(sk, lens, thr)
        # (the oracle clamps the NaN distance of 0 / 0 with Rust's f64::min and
        # f64::max, NaN lost: whether finch orders its clamp so is not pinned by the reference)
        both_empty = [(int(r["common"]), int(r["total"]), float(r["ani"])) for r in o
                      if int(r["i"]) in empty and int(r["j"]) in empty]
        assert both_empty == ([(0, 0, 0.0)] * 6 if thr == 0 else [])
        assert len(o) == 21 if thr == 0 else 1 <= len(o) <= 3
        pairs, ani = gpu_ctx.precluster_files(paths, thr)
        assert_pairs(pairs, quads(o), "min_ani=%r" % thr)
        assert ani.dtype == np.float32 and (ani == o["ani"]).all()
