"""The query of resident rows and of a resident collection:
hits and nearest representative of genomes that are not added.  Needs an
MI355X.

Expected values come from the CPU oracle, numpy, tests/cluster_ref.py and the
existing entry points only (tests/query_cases.py holds the scenarios and their
oracle reference).  Bar: (i, j, common, total) identical and in (i, j) order,
f32 ANI identical bit for bit.

A  every scenario through query_rows and query_rows_device
B  GALAHGPU_TEST_QUERY_BATCH = 1, 7, 63, 64 and unset: the same result
C  the capacity contract of the device form, both kernels behind it
D  min_ani 0.0 and -1.0: every cell, common == 0 and (0, 0) included
E  n == 0, nq == 0, n + nq == 2^31 and NaN
F  a collection is not changed by a query, at its own and at other thresholds
G  classify: galah's decision for the query appended last, ties, candidates
H  Collection.query on the golden files
"""
import numpy as np
import pytest

import cluster_ref
import galah_amd as ga
import query_cases as qc
from test_border_gpu import border_thresholds, golden_table
from test_collection_gpu import Handle
from test_pair_edges import (SENTINEL, SWEEP_S, assert_pairs, check_capacity_contract, pair_ani, quads,
                             sweep_reference, torch_dev)

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = 0xFFFFFFFF
INVALID = 1
THR = f32(0.9)


def bits_of(ani64):
    return np.asarray(ani64, dtype=np.float64).astype(np.float32).view(np.uint32)


def on_device(torch, case):
    return [torch.from_numpy(np.array(a, order="C").view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()
            for a in case]


def query_device_into(torch, ctx, dev, n, nq, thr, n_true, out_cap, initial, null_out=False):
    """One gg_query_rows_device call into a sentinel-filled buffer larger than
    any result -> (count after the call, the whole buffer [entries, 4])."""
    entries = max(out_cap, 5) + n_true + 64
    d_out = torch.full((entries * 4,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), initial, dtype=torch.int64, device="cuda")
    ctx.query_rows_device(dev[0], dev[1], n, dev[2], dev[3], nq, thr, None if null_out else d_out, out_cap, d_cnt)
    torch.cuda.synchronize()
    return int(d_cnt.item()), d_out.cpu().numpy().view(np.uint32).reshape(-1, 4)


def check_both_forms(torch, ctx, case, thr, exp, exp_ani64, what):
    sk, lens, q_sk, q_lens = case
    n, nq = len(lens), len(q_lens)
    pairs, ani = ctx.query_rows(sk, lens, q_sk, q_lens, thr)
    assert_pairs(pairs, exp, what)
    assert ani.dtype == np.float32 and (ani.view(np.uint32) == bits_of(exp_ani64)).all(), what
    count, buf = query_device_into(torch, ctx, on_device(torch, case), n, nq, thr, len(exp), len(exp) + 7, 0)
    assert count == len(exp) and (buf[count:] == SENTINEL).all(), what
    got = buf[:count]
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert (got == exp).all(), what


# ----------------------------------------------------------------------------
# A. every scenario, both forms
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 2])
def test_sweep_at_threshold_boundaries(k):
    """The sweep rows split 536 | 64, 599 | 1, 1 | 599 and 300 | 300 at 0.0, an
    achievable ANI value with its two f32 neighbours, and 0.95."""
    torch = torch_dev()
    _, _, v = sweep_reference(k)
    with ga.Context(k=k, sketch_size=SWEEP_S) as ctx:
        for thr in border_thresholds(v):
            passing = 0
            for n in qc.SWEEP_SPLITS:
                exp, exp_ani = qc.sweep_expected(n, thr, k)
                assert len(exp) == n * (600 - n) if thr == 0 else len(exp) < n * (600 - n)
                passing += len(exp)
                check_both_forms(torch, ctx, qc.sweep(n), thr, exp, exp_ani, "sweep %d k=%d min_ani=%r" % (n, k, thr))
            assert passing > 0, thr  # (a split of one row or one query may have no hit at a high threshold)


@pytest.mark.parametrize("name", [x for x in sorted(qc.CASES) if not x.startswith("sweep_")])
def test_scenarios(name):
    torch = torch_dev()
    fn, s = qc.CASES[name]
    exp = qc.expected(name, qc.bits(THR))
    assert name == "empty_queries" or len(exp) > 0
    if name == "large_s":
        assert exp[:, 2].max() == 12000  # the u16 counters reach the largest sketch size
    with ga.Context(k=21, sketch_size=s) as ctx:
        check_both_forms(torch, ctx, fn(), THR, exp, pair_ani(exp, 21) if len(exp) else np.zeros(0), name)


# ----------------------------------------------------------------------------
# B. the batch edge
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["1", "7", "63", "64", None])
def test_batches_give_the_same_result(monkeypatch, batch):
    if batch is None:
        monkeypatch.delenv("GALAHGPU_TEST_QUERY_BATCH", raising=False)
    else:
        monkeypatch.setenv("GALAHGPU_TEST_QUERY_BATCH", batch)
    _, _, v = sweep_reference(21)
    thr = border_thresholds(v)[2]
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx:
        ctx.timing_enable()
        exp, exp_ani = qc.sweep_expected(536, thr, 21)
        pairs, ani = ctx.query_rows(*qc.sweep(536), thr)
        assert_pairs(pairs, exp, "sweep, batches of %s" % batch)
        assert (ani.view(np.uint32) == bits_of(exp_ani)).all()
        launches = ctx.timing_read(ga.KERNEL_PAIRS)["launches"]
        assert launches == (1 if batch is None else -(-64 // int(batch))), launches  # 64 queries, one sized pass
    with ga.Context(k=21, sketch_size=64) as ctx:
        # (with batches of 1 the empty query is a batch of its own: nothing built, nothing found)
        exp = qc.expected("table", qc.bits(THR))
        pairs, ani = ctx.query_rows(*qc.table(), THR)
        assert_pairs(pairs, exp, "table, batches of %s" % batch)
        assert (ani.view(np.uint32) == bits_of(pair_ani(exp, 21))).all()


# ----------------------------------------------------------------------------
# C. capacity and append
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,thr,s", [("sweep_536", 0.9, SWEEP_S), ("table", 0.0, 64)])
def test_query_device_capacity_and_append(name, thr, s):
    """Output capacities below, at and above the result with *d_count starting
    at 0 and at 5, and a null output with out_cap = 0 (counting only): the
    stream kernel (min_ani 0.9) and the rectangle's append (min_ani 0)."""
    torch = torch_dev()
    case = qc.CASES[name][0]()
    n, nq = len(case[1]), len(case[3])
    true_set = set(map(tuple, qc.expected(name, qc.bits(thr)).tolist()))
    m = len(true_set)
    assert m >= 100
    dev = on_device(torch, case)
    with ga.Context(k=21, sketch_size=s) as ctx:
        for out_cap in (0, 1, m // 2, m - 1, m, m + 5):
            for initial in (0, 5):
                count, buf = query_device_into(torch, ctx, dev, n, nq, f32(thr), m, out_cap, initial)
                check_capacity_contract(count, buf, true_set, out_cap, initial, (name, out_cap, initial))
        for initial in (0, 5):
            count, buf = query_device_into(torch, ctx, dev, n, nq, f32(thr), m, 0, initial, null_out=True)
            assert count == initial + m and (buf == SENTINEL).all(), (name, "null output", initial)


# ----------------------------------------------------------------------------
# D. min_ani <= 0
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, -1.0])
def test_every_cell_at_zero(thr):
    torch = torch_dev()
    for name in ("table", "one_hash", "empty_queries"):
        fn, s = qc.CASES[name]
        case = fn()
        n, nq = len(case[1]), len(case[3])
        exp = qc.expected(name, qc.bits(thr))
        assert len(exp) == n * nq and (exp[:, 2] == 0).any() and ((exp[:, 2] == 0) & (exp[:, 3] == 0)).any()
        with ga.Context(k=21, sketch_size=s) as ctx:
            ctx.timing_enable()
            before = ctx.timing_read(ga.KERNEL_PAIRS)["launches"]
            check_both_forms(torch, ctx, case, f32(thr), exp, pair_ani(exp, 21), "%s at %r" % (name, thr))
            # the rectangle goes through the named-pair kernel, not the stream kernel
            assert ctx.timing_read(ga.KERNEL_PAIRS)["launches"] == before
            assert ctx.timing_read(ga.KERNEL_ANI_PAIRS)["launches"] == 2
        empty = (exp[:, 2] == 0) & (exp[:, 3] == 0)
        assert (bits_of(pair_ani(exp, 21))[empty] == 0).all()  # (0, 0): ANI 0


# ----------------------------------------------------------------------------
# E. limits
# ----------------------------------------------------------------------------
def test_limits():
    torch = torch_dev()
    sk, lens, q_sk, q_lens = qc.table()
    with ga.Context(k=21, sketch_size=64) as ctx:
        for a, b in (((sk[:0], lens[:0]), (q_sk, q_lens)), ((sk, lens), (q_sk[:0], q_lens[:0])),
                     ((sk[:0], lens[:0]), (q_sk[:0], q_lens[:0]))):
            pairs, ani = ctx.query_rows(*a, *b, THR)
            assert len(pairs) == 0 and len(ani) == 0
        dev = on_device(torch, (sk, lens, q_sk, q_lens))
        d_cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        ctx.query_rows_device(dev[0], dev[1], 0, dev[2], dev[3], len(q_lens), THR, None, 0, d_cnt)
        ctx.query_rows_device(dev[0], dev[1], len(lens), dev[2], dev[3], 0, THR, None, 0, d_cnt)
        torch.cuda.synchronize()
        assert int(d_cnt.item()) == 5
        for n, nq in ((2**31 - 1, 1), (1, 2**31 - 1), (2**30, 2**30)):  # refused before any array is read
            with pytest.raises(ga.GalahGpuError) as e:
                ctx.query_rows_device(dev[0], dev[1], n, dev[2], dev[3], nq, THR, None, 0, d_cnt)
            assert e.value.status == INVALID and "2^31" in str(e.value)
        for call in (lambda: ctx.query_rows(sk, lens, q_sk, q_lens, f32(np.nan)),
                     lambda: ctx.query_rows_device(dev[0], dev[1], len(lens), dev[2], dev[3], len(q_lens), f32(np.nan),
                                                   None, 0, d_cnt)):
            with pytest.raises(ga.GalahGpuError) as e:
                call()
            assert e.value.status == INVALID and "NaN" in str(e.value)
        long = q_lens.copy()
        long[0] = 65
        with pytest.raises(ga.GalahGpuError) as e:
            ctx.query_rows(sk, lens, q_sk, long, THR)
        assert e.value.status == INVALID
        assert int(d_cnt.item()) == 5


# ----------------------------------------------------------------------------
# F. a collection is only read
# ----------------------------------------------------------------------------
def snapshot(col):
    pairs, ani = col.pairs()
    rows, lens = col.rows()
    return col.ctx.collection_stat(col.h), col.view(), [pairs, ani, rows, lens]


def assert_same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all()


def test_a_query_leaves_the_collection(monkeypatch):
    sk, lens, q_sk, q_lens = qc.sweep(536)
    _, _, v = sweep_reference(21)
    inner = v[(v > 0) & (v < 1)]
    own, below, above = f32(inner[len(inner) // 2]), f32(inner[len(inner) // 4]), f32(inner[(3 * len(inner)) // 4])
    assert below < own < above
    with ga.Context(k=21, sketch_size=SWEEP_S) as ctx, Handle(ctx, own) as col:
        col.add_rows(sk[:300], lens[:300])
        col.add_rows(sk[300:], lens[300:])
        was = snapshot(col)
        assert was[0][0]["n_rows"] == 536 and was[0][0]["n_pairs"] > 0 and all(was[1])
        counters = ctx.pair_paths(), ctx.pairs_paths_taken(), ctx.fallbacks()
        ctx.timing_enable()
        launches = ctx.timing_read(ga.KERNEL_PAIRS)["launches"]
        for thr, env, expect in ((own, None, 1), (below, None, 1), (above, "7", 10)):
            if env:
                monkeypatch.setenv("GALAHGPU_TEST_QUERY_BATCH", env)
            exp, exp_ani = qc.sweep_expected(536, thr, 21)
            assert len(exp) > 0
            pairs, ani = col.query_rows(q_sk, q_lens, float(thr))
            assert_pairs(pairs, exp, "collection query at %r" % thr)
            assert (ani.view(np.uint32) == bits_of(exp_ani)).all()
            now = ctx.timing_read(ga.KERNEL_PAIRS)["launches"]
            assert now - launches == expect, (thr, now - launches)  # 64 queries, one sized pass
            launches = now
            assert_same(snapshot(col), was)
        best, best_ani = col.classify_rows(q_sk, q_lens)
        assert len(best) == 64 and (best["j"] == 536 + np.arange(64)).all()
        exp, exp_ani = qc.sweep_expected(536, own, 21)
        ref, ref_ani = ga.query_best_host(536, 64, exp_as_pairs(exp), exp_ani.astype(np.float32))
        assert (quads(best) == quads(ref)).all() and (best_ani.view(np.uint32) == ref_ani.view(np.uint32)).all()
        assert_same(snapshot(col), was)
        assert (ctx.pair_paths(), ctx.pairs_paths_taken(), ctx.fallbacks()) == counters
        assert col.info()["grows"] == was[0][0]["grows"]


def exp_as_pairs(q):
    pairs = np.zeros(len(q), ga.PAIR_DTYPE)
    for x, f in enumerate(("i", "j", "common", "total")):
        pairs[f] = q[:, x]
    return pairs


# ----------------------------------------------------------------------------
# G. classify
# ----------------------------------------------------------------------------
# of the 27 golden genomes: 0-17 are one species, 18-19, 20-21 and 22-26 without 24 three more, 24 is alone
QUERIED = [3, 8, 12, 19, 21, 24, 25]
OLD = [g for g in range(27) if g not in QUERIED]
N_OLD = len(OLD)


def decided_alone(q, ani, order, g, threshold):
    """galah's decision for golden genome g appended last to the collection's
    genomes (OLD) in `order`: None (a new representative) or (row of its
    representative, f32 ANI), from tests/cluster_ref.py on those 21."""
    pos = {OLD[int(row)]: p for p, row in enumerate(order)}
    pos[g] = N_OLD
    keep = [r for r in range(len(q)) if int(q[r, 0]) in pos and int(q[r, 1]) in pos]
    rel = np.array([(pos[int(q[r, 0])], pos[int(q[r, 1])]) for r in keep], dtype=np.uint32).reshape(-1, 2)
    rep = int(cluster_ref.cluster_ref(N_OLD + 1, rel, ani[keep], threshold)[N_OLD])
    if rep == N_OLD:
        return None
    row = int(order[rep])
    (a,) = [ani[r] for r in keep if {int(q[r, 0]), int(q[r, 1])} == {OLD[row], g}]
    return row, np.float32(a)


def test_classify_on_the_golden_genomes(golden, tmp_path):
    thr = ga.parse_percentage(90)
    assert len(golden["paths"]) == 27 and N_OLD == 20
    old, new = [golden["paths"][g] for g in OLD], [golden["paths"][g] for g in QUERIED]
    q, ani = golden_table(golden, thr)
    pre = ga.FinchPreclusterer(thr, sketch_cache_dir=str(tmp_path / "cache"))
    decisions = set()
    with pre.collection() as col:
        col.add(old)
        was = col.cache(), col.info()
        for order in (None, np.random.default_rng(5).permutation(N_OLD)):
            rows = np.arange(N_OLD) if order is None else order
            for T in (0.85, float(thr), 0.95, 0.99):  # below, at and above min_ani
                got = col.classify(new, ga.FinchClusterer(T), order=order)
                exp = [decided_alone(q, ani, rows, g, f32(T)) for g in QUERIED]
                assert len(got) == 7
                for g, e in zip(got, exp):
                    assert (g is None) == (e is None), (T, got, exp)
                    assert g is None or (g[0] == e[0] and f32(g[1]) == e[1]), (T, got, exp)
                decisions |= {(T, e is None) for e in exp}
        # members and new representatives were decided at every threshold, and the threshold moved some
        assert decisions == {(T, x) for T in (0.85, float(thr), 0.95, 0.99) for x in (True, False)}
        assert [decided_alone(q, ani, np.arange(N_OLD), 8, f32(T)) is None for T in (0.95, 0.99)] == [False, True]
        for call in (lambda: col.classify([new[1], str(tmp_path / "missing.fna")], ga.FinchClusterer(0.95)),
                     lambda: col.query([str(tmp_path / "missing.fna"), new[1]])):
            with pytest.raises(RuntimeError, match="Failed to sketch genomes with finch"):
                call()
        assert (col.cache(), col.info()) == was and col.paths == old
        # a genome of the collection finds itself
        (own,) = col.query(old[3:4])
        assert own[0] == (3, f32(1.0))


def test_classify_ties_and_candidates():
    rng = np.random.default_rng(31)
    s = 64
    v = np.unique(rng.integers(1, 2**44, 6 * s, dtype=np.uint64))
    a, b, z = v[:s], v[s:2 * s], v[4 * s:5 * s]
    near_a = np.concatenate([v[2:s], v[2 * s:2 * s + 2]])  # 62 of a's 64
    sk, lens = qc.matrix([a, b, a, v[3 * s:4 * s]], s)     # rows 0 and 2: bit-identical
    q_sk, q_lens = qc.matrix([near_a, z, []], s)
    with ga.Context(k=21, sketch_size=s) as ctx, Handle(ctx, THR) as col:
        col.add_rows(sk, lens)
        pairs, ani = col.query_rows(q_sk, q_lens, float(THR))
        assert [tuple(r) for r in quads(pairs)[:, :2].tolist()] == [(0, 4), (2, 4)] and ani[0] == ani[1]
        for rank, winner in ((None, 0), ([0, 1, 2, 3], 0), ([2, 1, 0, 3], 2), ([NONE, 1, 7, 3], 2), ([5, 1, NONE, 3], 0)):
            best, best_ani = col.classify_rows(q_sk, q_lens, rank=rank)
            assert int(best[0]["i"]) == winner and int(best[0]["j"]) == 4, (rank, best)
            assert (int(best[0]["common"]), int(best[0]["total"])) == (int(pairs[0]["common"]), int(pairs[0]["total"]))
            assert best_ani[0] == ani[0]
            assert [int(best[x]["i"]) for x in (1, 2)] == [NONE, NONE] and [int(best[x]["j"]) for x in (1, 2)] == [5, 6]
            assert (best_ani[1:] == 0).all()
        best, _ = col.classify_rows(q_sk, q_lens, rank=[NONE, 1, NONE, 3])  # the candidates that hit are none
        assert int(best[0]["i"]) == NONE
        with pytest.raises(ga.GalahGpuError) as e:
            col.classify_rows(q_sk, q_lens, rank=[1, 1, 2, 3])
        assert e.value.status == INVALID
        assert col.info()["n_rows"] == 4


# ----------------------------------------------------------------------------
# H. Collection.query
# ----------------------------------------------------------------------------
def test_collection_query_on_the_golden_genomes(golden):
    thr = ga.parse_percentage(90)
    old, new = [golden["paths"][g] for g in OLD], [golden["paths"][g] for g in QUERIED]
    pre = ga.FinchPreclusterer(thr)
    cache = ga.FinchPreclusterer(thr).distances(old + new)
    with pre.collection() as col:
        col.add(old)
        got = col.query(new)
        assert len(got) == 7 and sum(1 for h in got if h) >= 5 and got[5] == []  # (golden genome 24 is alone)
        for x, hits in enumerate(got):
            exp = [(i, f32(cache.get((i, N_OLD + x)))) for i in range(N_OLD) if cache.contains_key((i, N_OLD + x))]
            exp.sort(key=lambda h: (-float(h[1]), h[0]))
            assert [(i, f32(a)) for i, a in hits] == exp, x
        # a threshold of the call's own, above and below the collection's
        for own in (0.97, 0.8):
            q, ani = golden_table(golden, f32(own))
            hits = col.query(new, min_ani=own)
            for x, g in enumerate(QUERIED):
                exp = [(OLD.index(int(o)), a) for r, a in zip(q, ani) if g in (r[0], r[1])
                       for o in (r[0] + r[1] - g,) if int(o) in OLD]
                exp.sort(key=lambda h: (-float(h[1]), h[0]))
                assert [(i, f32(a)) for i, a in hits[x]] == exp, (own, x)
            assert (sum(len(h) for h in hits) < sum(len(h) for h in got)) == (own > thr)
        assert len(col) == N_OLD and col.cache() == ga.FinchPreclusterer(thr).distances(old)
