"""The Python binding at the device, pinned before its call frame was shared
(DESIGN.md 4.18).  Needs an MI355X.

What a caller of galah_amd.Context (and of Collection and FinchPreclusterer
above it) can observe, on a one-device context and on the two-member context
over one device ([0, 0]), with test_call_frame_gpu's Env (k = 21, sketch size
32, 3 rows, three files of 400 bases):

  (a) a refusal reachable from Python: the exception's class, its .status and
      the whole of str(e); for the two files calls also ctx.last_cached;
  (b) the same method called validly straight afterwards on the same context,
      equal to the host form where one exists;
  (c) the method at n == 0 (no paths, no rows, no pairs, no queries, no
      genome in any shard): dtype and shape of every returned value.  Beside
      each method's (a) and (b) where the library returns before any device
      work; test_no_input holds the calls that go on into their device code
      with nothing to do (the files forms, the validation, the pair matrix
      forms, gg_preclusters, the collection's load, remove and query_rows).
      Each was read in the source first: an empty input is an ordinary call.

test_precluster_shards is the call inside bench.py's timed step;
test_collection_class runs class Collection's methods and pins the texts of
its own checks (a path present, an order that is no permutation, another
clusterer, a state of other parameters).

Every class, status and message was read from the Python of commit 68eb3f2
and from the fail() / check_*() texts of galah_amd/csrc (the same texts
tests/test_call_frame_gpu.py pins at the C ABI); nothing was taken from what a
run printed.  The same file passes on that commit's module and on this tree's.

No case asks the device to fault: every refusal is a host-side check before any
launch, one of Python's own argument checks, or an ordinary file error.
"""
import numpy as np
import pytest

import galah_amd as ga
from test_call_frame_gpu import (CLUSTERS, GROUP_MEMBERS, GROUP_OFFSETS, K, MIN_ANI, N, NAN, S, Col, Env,
                                 assert_matrix, assert_rows_from_files, assert_validation, dev, exp_partition, exp_rep,
                                 f32_bits, host, named_list, pair_ani, same_pairs)
from test_pair_edges import torch_dev

pytestmark = pytest.mark.gpu

INVALID, IO, CANCELLED = 1, 2, 9
CONTEXTS = {"one": [0], "two": [0, 0]}
EMPTY_SK, EMPTY_LENS = np.zeros((0, S), np.uint64), np.zeros(0, np.uint32)


@pytest.fixture(scope="module", params=sorted(CONTEXTS))
def env(request, tmp_path_factory):
    e = Env(CONTEXTS[request.param], str(tmp_path_factory.mktemp("binding_frame")))
    yield e
    e.close()


def refused(status, message, fn, *args, **kw):
    with pytest.raises(ga.GalahGpuError) as x:
        fn(*args, **kw)
    assert type(x.value) is ga.GalahGpuError and x.value.status == status
    assert str(x.value) == "%s (status %d)" % (message, status)


def value_error(text, fn, *args, **kw):
    with pytest.raises(ValueError) as x:
        fn(*args, **kw)
    assert type(x.value) is ValueError and str(x.value) == text


def shapes(*arrays):
    return [(a.dtype, a.shape) for a in arrays]


PAIRS0, F32_0, U32_0 = (ga.PAIR_DTYPE, (0,)), (np.dtype(np.float32), (0,)), (np.dtype(np.uint32), (0,))
ROWS0 = [(np.dtype(np.uint64), (0, S)), U32_0]


# ---- rows in host memory -------------------------------------------------------------
def test_pairs_and_borders(env):
    e, ctx = env, env.ctx
    refused(INVALID, "sketch longer than sketch_size", ctx.pairs, e.sk, e.long_lens, MIN_ANI)
    assert same_pairs(ctx.pairs(e.sk, e.lens, MIN_ANI), e.exp)
    value_error("sketches must be [n, sketch_size]", ctx.pairs, e.sk[:, :S - 1], e.lens, MIN_ANI)
    assert shapes(ctx.pairs(EMPTY_SK, EMPTY_LENS, MIN_ANI)) == [PAIRS0]

    refused(INVALID, "gg_pairs_border: n_old exceeds n", ctx.pairs_border, e.sk, e.lens, N + 1, MIN_ANI)
    refused(INVALID, "sketch longer than sketch_size", ctx.pairs_border, e.sk, e.long_lens, 1, MIN_ANI)
    assert same_pairs(ctx.pairs_border(e.sk, e.lens, 1, MIN_ANI), ga.pairs_border_host(e.sk, e.lens, 1, MIN_ANI, k=K))
    assert shapes(ctx.pairs_border(EMPTY_SK, EMPTY_LENS, 0, MIN_ANI)) == [PAIRS0]
    assert shapes(ctx.pairs_border(e.sk, e.lens, N, MIN_ANI)) == [PAIRS0]  # (no new row)

    refused(INVALID, "gg_pairs_matrix: row index listed twice", ctx.pairs_matrix, e.sk, e.lens, MIN_ANI, rows=[0, 1, 1])
    pairs, summary = ctx.pairs_matrix(e.sk, e.lens, MIN_ANI)
    assert same_pairs(pairs, e.exp) and summary["n_pairs"] == 1 and summary["path"] in ga.PAIRS_PATHS
    assert sorted(summary) == sorted(f for f, _ in ga._PairsMatrixSummary._fields_)
    pairs, _ = ctx.pairs_matrix(e.sk, e.lens, MIN_ANI, rows=np.array([1, 0], np.uint32))
    assert pairs.dtype == ga.PAIR_DTYPE and len(pairs) == 1

    refused(INVALID, "gg_pairs_border_matrix: n_old exceeds n", ctx.pairs_border_matrix, e.sk, e.lens, N + 1, MIN_ANI)
    pairs, summary = ctx.pairs_border_matrix(e.sk, e.lens, 1, MIN_ANI)
    assert same_pairs(pairs, ga.pairs_border_host(e.sk, e.lens, 1, MIN_ANI, k=K)) and summary["n_pairs"] == 1


def test_update_files(env):
    e, ctx = env, env.ctx
    old_sk, old_lens = e.fsk[[0, 2]], e.flens[[0, 2]]
    refused(IO, e.io_message, ctx.update_files, old_sk, old_lens, [e.paths[1], e.missing[0]], MIN_ANI)
    refused(INVALID, "sketch longer than sketch_size", ctx.update_files, old_sk, [S + 1, 20], e.paths[1:2], MIN_ANI)
    new_sk, new_lens, pairs, ani = ctx.update_files(old_sk, old_lens, e.paths[1:2], MIN_ANI)
    exp = ga.pairs_border_host(e.fsk[[0, 2, 1]], e.flens[[0, 2, 1]], 2, MIN_ANI, k=K)
    assert (new_sk[0] == e.fsk[1]).all() and new_lens.tolist() == [e.flens[1]]
    assert same_pairs(pairs, exp) and f32_bits(ani) == f32_bits(pair_ani(exp)) and len(exp) == 1
    out = ctx.update_files(old_sk, old_lens, [], MIN_ANI)  # no new file
    assert shapes(*out) == ROWS0 + [PAIRS0, F32_0]


def test_cluster_preclusters_ani_pairs(env):
    e, ctx = env, env.ctx
    refused(INVALID, "gg_cluster_pairs: cluster_ani is NaN", ctx.cluster_pairs, N, e.exp, e.exp_ani, NAN)
    value_error("one ani per pair", ctx.cluster_pairs, N, e.exp, [0.9, 0.9], MIN_ANI)
    assert ctx.cluster_pairs(N, e.exp, e.exp_ani, MIN_ANI).tolist() == exp_rep(e).tolist()
    assert shapes(ctx.cluster_pairs(0, [], [], MIN_ANI)) == [U32_0]

    bad = e.exp.copy()
    bad["i"] = N
    refused(INVALID, "gg_preclusters: pair index out of range", ctx.preclusters, N, bad)
    members, offsets, local, poff = ctx.preclusters(N, e.exp)
    em, eo = exp_partition(e)
    el, ep = ga.precluster_pairs(N, e.exp, em, eo)
    assert members.tolist() == em.tolist() and offsets.tolist() == eo.tolist()
    assert local.tolist() == el.tolist() and poff.tolist() == ep.tolist()
    assert shapes(members, offsets, local, poff) == shapes(em, eo, el, ep)
    members, offsets, local, poff = ctx.preclusters(N, e.exp, with_pairs=False)
    assert members.tolist() == em.tolist() and offsets.tolist() == eo.tolist() and local is None and poff is None

    bad = named_list()
    bad["j"][1] = N
    refused(INVALID, "gg_ani_pairs: pair index out of range", ctx.ani_pairs, e.sk, e.lens, bad)
    refused(INVALID, "gg_ani_pairs: sketch longer than sketch_size", ctx.ani_pairs, e.sk, e.long_lens, named_list())
    got, ani = ctx.ani_pairs(e.sk, e.lens, named_list())
    exp, exp_ani = ga.ani_pairs_host(e.sk, e.lens, named_list(), k=K)
    assert same_pairs(got, exp) and f32_bits(ani) == f32_bits(exp_ani)
    assert shapes(*ctx.ani_pairs(e.sk, e.lens, [])) == [PAIRS0, F32_0]


MATRIX0 = [(np.dtype(np.uint32), (0, 0)), (np.dtype(np.uint32), (0, 0)), (np.dtype(np.float32), (0, 0))]
MATRIX_KEYS = sorted(f for f, _ in ga._MatrixSummary._fields_)


def test_matrices(env):
    e, ctx = env, env.ctx
    refused(INVALID, "gg_ani_matrix: row index out of range", ctx.ani_matrix, e.sk, e.lens, rows=[0, N])
    got = ctx.ani_matrix(e.sk, e.lens)
    assert_matrix(got, ga.ani_matrix_host(e.sk, e.lens, k=K))
    assert sorted(got[3]) == MATRIX_KEYS and all(type(v) is int for v in got[3].values())
    got = ctx.ani_matrix(e.sk, e.lens, rows=[])
    assert shapes(*got[:3]) == MATRIX0 and got[3] == dict.fromkeys(got[3], 0) and sorted(got[3]) == MATRIX_KEYS

    refused(INVALID, "gg_ani_matrix_groups: row index out of range", ctx.ani_matrix_groups, e.sk, e.lens, [[1, N], [2]])
    value_error("offsets must have n_groups + 1 entries and end within members", ctx.ani_matrix_groups, e.sk, e.lens,
                [0, 1], [0, 3])
    got = ctx.ani_matrix_groups(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS)
    exp = ga.ani_matrix_groups_host(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS, k=K)
    assert_matrix(got, exp)
    assert got[3].tolist() == exp[3].tolist() and sorted(got[4]) == MATRIX_KEYS
    got = ctx.ani_matrix_groups(e.sk, e.lens, [])
    assert shapes(*got[:3]) == [U32_0, U32_0, F32_0] and got[3].tolist() == [0] and got[3].dtype == np.uint64

    refused(IO, e.io_message, ctx.ani_matrix_files, e.bad_paths)
    assert_matrix(ctx.ani_matrix_files(e.paths), ga.ani_matrix_host(e.fsk, e.flens, k=K))
    got = ctx.ani_matrix_files([])
    assert shapes(*got[:3]) == MATRIX0 and sorted(got[3]) == MATRIX_KEYS


def test_validation(env):
    e, ctx = env, env.ctx
    refused(INVALID, "gg_validate_clusters: ani is NaN", ctx.validate_clusters, e.sk, e.lens, CLUSTERS, NAN)
    exp = ga.validate_clusters_host(e.sk, e.lens, CLUSTERS, 0.9999, k=K)
    got = ctx.validate_clusters(e.sk, e.lens, CLUSTERS, 0.9999)
    assert type(got) is ga.Validation and exp.member_bad == 1
    assert_validation(got, exp)
    refused(IO, e.io_message, ctx.validate_files, e.bad_paths, CLUSTERS, 0.9999)
    assert_validation(ctx.validate_files(e.paths, CLUSTERS, 0.9999),
                      ga.validate_clusters_host(e.fsk, e.flens, CLUSTERS, 0.9999, k=K))


def test_queries(env):
    e, ctx = env, env.ctx
    q_sk, q_lens = e.sk[:1], e.lens[:1]  # row 0 asked again: it finds itself and row 1
    exp = ga.query_host(e.sk, e.lens, q_sk, q_lens, MIN_ANI, k=K)
    assert [(int(p["i"]), int(p["j"])) for p in exp] == [(0, N), (1, N)]
    refused(INVALID, "gg_query_rows: sketch longer than sketch_size", ctx.query_rows, e.sk, e.lens, q_sk, [S + 1], MIN_ANI)
    pairs, ani = ctx.query_rows(e.sk, e.lens, q_sk, q_lens, MIN_ANI)
    assert same_pairs(pairs, exp) and f32_bits(ani) == f32_bits(pair_ani(exp))
    assert shapes(*ctx.query_rows(e.sk, e.lens, EMPTY_SK, EMPTY_LENS, MIN_ANI)) == [PAIRS0, F32_0]
    assert shapes(*ctx.query_rows(EMPTY_SK, EMPTY_LENS, q_sk, q_lens, MIN_ANI)) == [PAIRS0, F32_0]


# ---- files -----------------------------------------------------------------------------
def test_sketch_files(env):
    e, ctx = env, env.ctx
    refused(IO, e.io_message, ctx.sketch_files, e.bad_paths)
    sk, lens, hits = ctx.sketch_files(e.paths)
    assert_rows_from_files(e, sk, lens)
    assert hits == 0 and shapes(sk, lens) == [(np.dtype(np.uint64), (N, S)), (np.dtype(np.uint32), (N,))]
    sk, lens, hits = ctx.sketch_files([])
    assert shapes(sk, lens) == ROWS0 and hits == 0

    refused(IO, e.io_message, ctx.sketch_files_stats, e.bad_paths)
    sk, lens, stats = ctx.sketch_files_stats(e.paths)
    assert_rows_from_files(e, sk, lens)
    assert stats == [ga.calculate_genome_stats(p) for p in e.paths]
    sk, lens, stats = ctx.sketch_files_stats([])
    assert shapes(sk, lens) == ROWS0 and stats == []


def test_precluster_files(env):
    """last_cached is written before the status is looked at: on a refusal too."""
    e, ctx = env, env.ctx
    for status, message, paths, min_ani in ((INVALID, "min_ani is NaN", e.paths, NAN),
                                            (IO, e.io_message, e.bad_paths, MIN_ANI)):
        ctx.last_cached = 7
        refused(status, message, ctx.precluster_files, paths, min_ani)
        assert ctx.last_cached == 0
        ctx.last_cached = 7
        refused(status, message, ctx.precluster_files_each, paths, min_ani, lambda blk: False)
        assert ctx.last_cached == 0
    ctx.last_cached = 7
    pairs, ani = ctx.precluster_files(e.paths, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani) and ctx.last_cached == 0


def test_precluster_files_each(env):
    e, ctx = env, env.ctx

    class Stop(Exception):
        pass

    def raises(blk):
        raise Stop("from the callback")

    ctx.last_cached = 7
    with pytest.raises(Stop, match="^from the callback$"):  # the callback's exception, not GalahGpuError
        ctx.precluster_files_each(e.paths, MIN_ANI, raises)
    assert ctx.last_cached == 0
    ctx.last_cached = 7
    refused(CANCELLED, "gg_precluster_files_each: the pair sink stopped the call", ctx.precluster_files_each, e.paths,
            MIN_ANI, lambda blk: True)
    assert ctx.last_cached == 0
    blocks = []
    pairs, ani = ctx.precluster_files_each(e.paths, MIN_ANI, lambda blk: blocks.append(blk.copy()) and False)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    every = ga.pairs_border_host(e.fsk, e.flens, 0, 0.0, k=K)
    assert all(b.dtype == ga.PAIR_DTYPE for b in blocks) and same_pairs(np.concatenate(blocks), every) and len(every) == 3


def test_resident_files_calls(env):
    e, ctx = env, env.ctx
    refused(INVALID, "gg_precluster_files_resident: min_ani is NaN", ctx.precluster_files_resident, e.paths, NAN)
    refused(IO, e.io_message, ctx.precluster_files_resident, e.bad_paths, MIN_ANI)
    pairs, ani, summary = ctx.precluster_files_resident(e.paths, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    assert summary["n_pairs"] == 1 and summary["path"] == "default"
    pairs, ani, summary = ctx.precluster_files_resident([], MIN_ANI)
    assert shapes(pairs, ani) == [PAIRS0, F32_0] and summary == ga._PairsMatrixSummary().as_dict()

    refused(INVALID, "gg_precluster_matrices_files: min_ani is NaN", ctx.precluster_matrices_files, e.paths, NAN)
    refused(IO, e.io_message, ctx.precluster_matrices_files, e.bad_paths, MIN_ANI)
    members, offsets, cells, common, total, ani, summary = ctx.precluster_matrices_files(e.paths, MIN_ANI)
    assert members.tolist() == [0, 1, 2] and offsets.tolist() == [0, 2, 3] and cells.tolist() == [0, 4, 5]
    c, t, a = ga.ani_matrix_groups_host(e.fsk, e.flens, members, offsets, k=K)[:3]
    assert common.tolist() == c.tolist() and total.tolist() == t.tolist() and f32_bits(ani) == f32_bits(a)
    assert shapes(members, offsets, cells, common, total, ani) == shapes(
        np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint64), c, t, a)
    assert sorted(summary) == MATRIX_KEYS
    members, offsets, cells, common, total, ani, summary = ctx.precluster_matrices_files([], MIN_ANI)
    assert shapes(members, common, total, ani) == [U32_0, U32_0, U32_0, F32_0]
    assert shapes(offsets, cells) == [(np.dtype(np.uint32), (1,)), (np.dtype(np.uint64), (1,))]

    refused(INVALID, "gg_cluster_files: null rep_of or NaN cluster_ani", ctx.cluster_files, e.paths, MIN_ANI, NAN)
    refused(IO, e.io_message, ctx.cluster_files, e.bad_paths, MIN_ANI, MIN_ANI)
    rep, pairs, ani = ctx.cluster_files(e.paths, MIN_ANI, MIN_ANI)
    exp_rep_f = ga.cluster_pairs_host(N, e.fexp, e.fexp_ani, MIN_ANI)
    assert rep.tolist() == exp_rep_f.tolist() == [0, 0, 2] and rep.dtype == np.uint32
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    rep = ctx.cluster_files(e.paths, MIN_ANI, MIN_ANI, want_pairs=False)
    assert type(rep) is np.ndarray and rep.tolist() == [0, 0, 2]

    refused(INVALID, "gg_cluster_files_resident: min_ani or cluster_ani is NaN", ctx.cluster_files_resident, e.paths,
            MIN_ANI, NAN)
    refused(IO, e.io_message, ctx.cluster_files_resident, e.bad_paths, MIN_ANI, MIN_ANI)
    rep, summary = ctx.cluster_files_resident(e.paths, MIN_ANI, MIN_ANI)
    assert rep.tolist() == [0, 0, 2] and summary["n_pairs"] == 1 and summary["n_preclusters"] == 2
    assert sorted(summary) == sorted(f for f, _ in ga._ClusterSummary._fields_ if f != "reserved")
    rep, summary = ctx.cluster_files_resident([], MIN_ANI, MIN_ANI)
    assert shapes(rep) == [U32_0] and summary == dict.fromkeys(summary, 0)


# ---- the collection ------------------------------------------------------------------------
def test_collection_calls(env):
    e, ctx = env, env.ctx
    refused(INVALID, "gg_collection_create: min_ani is NaN", ctx.collection_create, NAN)
    unsorted = np.zeros(2, ga.PAIR_DTYPE)
    unsorted["i"], unsorted["j"] = [0, 0], [2, 1]
    refused(INVALID, "gg_collection_load: the pairs are not strictly ascending by (i, j)", ctx.collection_load, e.sk,
            e.lens, unsorted, [0.95, 0.95], MIN_ANI)
    value_error("one ANI value per pair", ctx.collection_load, e.sk, e.lens, e.exp, [0.95, 0.95], MIN_ANI)
    h = ctx.collection_load(e.sk, e.lens, e.exp, e.exp_ani, MIN_ANI)
    assert type(h) is int
    pairs, ani = ctx.collection_pairs(h)
    assert same_pairs(pairs, e.exp) and f32_bits(ani) == f32_bits(e.exp_ani)
    ctx.collection_destroy(h)

    with Col(e, rows=0) as col:  # an empty collection
        assert type(col.h) is int
        assert ctx.collection_add_rows(col.h, EMPTY_SK, EMPTY_LENS) == 0 and ctx.collection_add_files(col.h, []) == 0
        assert shapes(*ctx.collection_rows(col.h)) == ROWS0
        assert shapes(ctx.collection_cluster(col.h, MIN_ANI)) == [U32_0]
        info, thr = ctx.collection_stat(col.h)
        assert sorted(info) == sorted(f for f, _ in ga._CollectionInfo._fields_) and info["n_rows"] == 0
        assert type(thr) is np.float32 and thr == np.float32(MIN_ANI)

    with Col(e, rows=2) as col:
        refused(INVALID, "gg_collection_add_rows: sketch longer than sketch_size", ctx.collection_add_rows, col.h,
                e.sk[2:], [S + 1])
        assert ctx.collection_add_rows(col.h, e.sk[2:], e.lens[2:]) == 0
        col.assert_unchanged()
        view = ctx.collection_view(col.h)
        assert len(view) == 4 and all(type(p) is int for p in view) and view[0] and view[1]

    with Col(e, rows=1) as col:
        assert ctx.collection_add_rows_device(col.h, dev(e.sk[1:]), dev(e.lens[1:]), 2) == 1
        col.assert_unchanged()

    with Col(e, rows=0) as col:
        refused(IO, e.io_message, ctx.collection_add_files, col.h, e.bad_paths)
        assert ctx.collection_stat(col.h)[0]["n_rows"] == 0
        assert ctx.collection_add_files(col.h, e.paths) == 1
        col.assert_is(e.fsk, e.flens, e.fexp, e.fexp_ani)

    with Col(e) as col:
        refused(INVALID, "gg_collection_remove: row index out of range", ctx.collection_remove, col.h, [2, N])
        value_error("order must be a permutation of 0 .. 2", ctx.collection_cluster, col.h, MIN_ANI, [0, 1])
        refused(INVALID, "gg_collection_cluster: order is not a permutation", ctx.collection_cluster, col.h, MIN_ANI,
                [0, 1, 1])
        col.assert_unchanged()
        order = np.array([2, 1, 0], np.uint32)
        exp = ga.cluster_pairs_host(N, ga.relabel_pairs(e.exp, order), e.exp_ani, MIN_ANI)
        assert ctx.collection_cluster(col.h, MIN_ANI, order).tolist() == exp.tolist()
        assert ctx.collection_cluster(col.h, MIN_ANI).tolist() == exp_rep(e).tolist()
        new_index = ctx.collection_remove(col.h, [2])
        assert new_index.dtype == np.uint32 and new_index.tolist() == [0, 1, 0xFFFFFFFF]
        col.assert_is(e.sk[:2], e.lens[:2], e.exp, e.exp_ani)


def test_collection_queries(env):
    e, ctx = env, env.ctx
    q_sk, q_lens = e.sk[:1], e.lens[:1]
    exp = ga.query_host(e.sk, e.lens, q_sk, q_lens, MIN_ANI, k=K)
    exp_ani = pair_ani(exp)
    exp_best, exp_best_ani = ga.query_best_host(N, 1, exp, exp_ani)
    fexp = ga.query_host(e.fsk, e.flens, e.fsk[:1], e.flens[:1], MIN_ANI, k=K)
    fbest, fbest_ani = ga.query_best_host(N, 1, fexp, pair_ani(fexp))
    with Col(e) as col:
        refused(INVALID, "gg_collection_query_rows: min_ani is NaN", ctx.collection_query_rows, col.h, q_sk, q_lens, NAN)
        pairs, ani = ctx.collection_query_rows(col.h, q_sk, q_lens, MIN_ANI)
        assert same_pairs(pairs, exp) and f32_bits(ani) == f32_bits(exp_ani)

        value_error("one rank per row", ctx.collection_classify_rows, col.h, q_sk, q_lens, rank=[0, 1])
        refused(INVALID, "gg_collection_classify_rows: sketch longer than sketch_size", ctx.collection_classify_rows,
                col.h, q_sk, [S + 1])
        best, best_ani = ctx.collection_classify_rows(col.h, q_sk, q_lens)
        assert same_pairs(best, exp_best) and f32_bits(best_ani) == f32_bits(exp_best_ani)
        assert shapes(*ctx.collection_classify_rows(col.h, EMPTY_SK, EMPTY_LENS)) == [PAIRS0, F32_0]
        col.assert_unchanged()

    with Col(e, rows=0) as col:
        assert ctx.collection_add_files(col.h, e.paths) == 1
        refused(IO, e.io_message, ctx.collection_query_files, col.h, e.bad_paths, MIN_ANI)
        pairs, ani = ctx.collection_query_files(col.h, e.paths[:1], MIN_ANI)
        assert same_pairs(pairs, fexp) and f32_bits(ani) == f32_bits(pair_ani(fexp))
        pairs, ani, sk, lens = ctx.collection_query_files(col.h, e.paths[:1], MIN_ANI, want_sketches=True)
        assert same_pairs(pairs, fexp) and (sk[0] == e.fsk[0]).all() and lens.tolist() == [e.flens[0]]
        assert shapes(*ctx.collection_query_files(col.h, [], MIN_ANI)) == [PAIRS0, F32_0]
        assert shapes(*ctx.collection_query_files(col.h, [], MIN_ANI, want_sketches=True)) == [PAIRS0, F32_0] + ROWS0

        value_error("one rank per row", ctx.collection_classify_files, col.h, e.paths[:1], rank=[0])
        refused(IO, e.io_message, ctx.collection_classify_files, col.h, e.bad_paths)
        best, best_ani = ctx.collection_classify_files(col.h, e.paths[:1])
        assert same_pairs(best, fbest) and f32_bits(best_ani) == f32_bits(fbest_ani)
        assert shapes(*ctx.collection_classify_files(col.h, [])) == [PAIRS0, F32_0]
        col.assert_is(e.fsk, e.flens, e.fexp, e.fexp_ani)


# ---- the read-outs and the settings ----------------------------------------------------------
def test_read_outs(env):
    ctx = env.ctx
    ctx.pairs(env.sk, env.lens, MIN_ANI)
    phases = ctx.phase_times()
    assert sorted(phases) == sorted(ga.PHASES) and all(type(v) is float for v in phases.values())
    paths = ctx.pair_paths()
    assert sorted(paths) == ["gate", "index", "index_abandoned", "index_full_sort", "other"]
    assert all(type(v) is int for v in paths.values())
    fallbacks = ctx.fallbacks()
    assert sorted(fallbacks) == sorted(ga.FALLBACKS) and all(type(v) is int for v in fallbacks.values())
    links = ctx.peer_links()
    assert links.dtype == np.int32 and links.shape == (ctx.device_count,) * 2
    assert type(ctx.info_line()) is str and ctx.info_line().startswith("galahgpu: ")
    stats = ctx.timing_read(ga.KERNEL_PAIRS)
    assert sorted(stats) == ["launches", "ms", "work"] and type(stats["ms"]) is float and type(stats["launches"]) is int
    taken = ctx.pairs_paths_taken()
    assert sorted(taken) == sorted(ga.PAIRS_PATHS) and all(type(v) is int for v in taken.values())
    assert ctx.pairs_path == "default" and type(ctx.device) is int and ctx.device_count == len(ctx.peer_links())
    assert ctx.timing_enable(False) is None and ctx.set_host_threads(2) is None and ctx.set_host_threads(0) is None


def test_set_pairs_path(env):
    ctx = env.ctx
    value_error("pairs path must be one of default, matrix, auto, not 'fast'", ctx.set_pairs_path, "fast")
    assert ctx.pairs_path == "default"
    assert ctx.set_pairs_path("auto") == "default" and ctx.pairs_path == "auto"
    assert ctx.set_pairs_path("default") == "auto" and ctx.pairs_path == "default"


# ---- the device forms: tensors and stream=None; two of them with pointers and a stream ---------
def test_device_forms(env):
    e, ctx, torch = env, env.ctx, torch_dev()
    pk = ga.pack_records([[s] for s in e.seqs], k=K)
    d_words = dev(pk.words).view(torch.int32)
    d_sk, d_len = dev(np.zeros((N, S), np.uint64)), dev(np.zeros(N, np.uint32))
    assert ctx.sketch_device(d_words, pk.runs.copy(), N, d_sk, d_len) is None
    assert_rows_from_files(e, host(d_sk, np.uint64).reshape(N, S), host(d_len, np.uint32))
    sk, lens = ctx.sketch(pk)
    assert_rows_from_files(e, sk, lens)
    assert shapes(*ctx.sketch(ga.pack_records([], k=K))) == ROWS0

    def outputs():
        return dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64))

    def one_pair(d_out, d_count, exp):
        torch.cuda.synchronize()
        return host(d_count, np.uint64)[0] == len(exp) and same_pairs(host(d_out, ga.PAIR_DTYPE)[:len(exp)], exp)

    d_out, d_count = outputs()
    assert ctx.pairs_device(e.d_sk, e.d_lens, N, 0, ga.pair_tiles(N), MIN_ANI, d_out, 4, d_count) is None
    assert one_pair(d_out, d_count, e.exp)

    refused(INVALID, "gg_pairs_border_device: n_old exceeds n", ctx.pairs_border_device, e.d_sk, e.d_lens, N, N + 1,
            MIN_ANI, d_out, 4, d_count)
    d_out, d_count = outputs()
    ctx.pairs_border_device(e.d_sk, e.d_lens, N, 1, MIN_ANI, d_out, 4, d_count)
    assert one_pair(d_out, d_count, e.exp)

    d_pairs, d_ani, d_rep = dev(e.exp), dev(e.exp_ani), dev(np.full(N, 7, np.uint32))
    refused(INVALID, "gg_cluster_pairs_device: cluster_ani is NaN", ctx.cluster_pairs_device, N, d_pairs, d_ani, 1, NAN,
            d_rep)
    assert host(d_rep, np.uint32).tolist() == [7] * N
    ctx.cluster_pairs_device(N, d_pairs, d_ani, 1, MIN_ANI, d_rep)
    assert host(d_rep, np.uint32).tolist() == exp_rep(e).tolist()

    d_val = dev(np.zeros(1, np.float32))
    assert type(ctx.ani_f32_device(d_pairs, 1, d_val)) is int
    assert f32_bits(host(d_val, np.float32)) == f32_bits(e.exp_ani)

    d_rep = dev(np.full(N, 7, np.uint32))
    refused(INVALID, "gg_cluster_rows_device: min_ani or cluster_ani is NaN", ctx.cluster_rows_device, e.d_sk, e.d_lens, N,
            NAN, MIN_ANI, d_rep)
    summary, p, a, n_pairs = ctx.cluster_rows_device(e.d_sk, e.d_lens, N, MIN_ANI, MIN_ANI, d_rep)
    assert host(d_rep, np.uint32).tolist() == exp_rep(e).tolist() and n_pairs == 1 and type(p) is int and type(a) is int
    assert summary["n_preclusters"] == 2 and "reserved" not in summary
    summary, p, a, n_pairs = ctx.cluster_rows_device(e.d_sk, e.d_lens, N, MIN_ANI, MIN_ANI, d_rep, want_summary=False)
    assert summary is None and n_pairs is None and p and a

    d_members, d_offsets = dev(np.full(N, 7, np.uint32)), dev(np.full(N + 1, 7, np.uint32))
    assert ctx.preclusters_device(N, d_pairs, 1, d_members, d_offsets) == 2
    em, eo = exp_partition(e)
    assert host(d_members, np.uint32).tolist() == em.tolist() and host(d_offsets, np.uint32)[:3].tolist() == eo.tolist()

    d_list = dev(named_list())
    assert ctx.ani_pairs_device(e.d_sk, e.d_lens, N, d_list, 2) is None
    torch.cuda.synchronize()
    assert same_pairs(host(d_list, ga.PAIR_DTYPE), ga.ani_pairs_host(e.sk, e.lens, named_list(), k=K)[0])

    d_out, d_count = outputs()
    refused(INVALID, "gg_pairs_matrix_device: min_ani is NaN", ctx.pairs_matrix_device, e.d_sk, e.d_lens, N, None, N, NAN,
            d_out, 4, d_count)
    summary = ctx.pairs_matrix_device(e.d_sk, e.d_lens, N, None, N, MIN_ANI, d_out, 4, d_count)
    assert one_pair(d_out, d_count, e.exp) and summary["n_pairs"] == 1 and summary["path"] == "matrix"
    d_out, d_count = outputs()
    assert ctx.pairs_matrix_device(e.d_sk, e.d_lens, N, None, N, MIN_ANI, d_out, 4, d_count, want_summary=False) is None
    assert one_pair(d_out, d_count, e.exp)

    d_out, d_count = outputs()
    refused(INVALID, "gg_pairs_border_matrix_device: n_old exceeds n", ctx.pairs_border_matrix_device, e.d_sk, e.d_lens, N,
            N + 1, MIN_ANI, d_out, 4, d_count)
    summary = ctx.pairs_border_matrix_device(e.d_sk, e.d_lens, N, 1, MIN_ANI, d_out, 4, d_count)
    assert one_pair(d_out, d_count, e.exp) and summary["n_pairs"] == 1

    refused(INVALID, "gg_ani_matrix_device: no output asked for", ctx.ani_matrix_device, e.d_sk, e.d_lens, N, None, N)
    d = [dev(np.full(N * N, 7, t)) for t in (np.uint32, np.uint32, np.float32)]
    summary = ctx.ani_matrix_device(e.d_sk, e.d_lens, N, None, N, *d)
    got = (host(d[0], np.uint32), host(d[1], np.uint32), host(d[2], np.float32))
    assert_matrix(got, [x.reshape(-1) for x in ga.ani_matrix_host(e.sk, e.lens, k=K)])
    assert sorted(summary) == MATRIX_KEYS

    d = [dev(np.full(5, 7, t)) for t in (np.uint32, np.uint32, np.float32)]
    summary = ctx.ani_matrix_groups_device(e.d_sk, e.d_lens, N, dev(GROUP_MEMBERS), GROUP_OFFSETS, *d)
    got = (host(d[0], np.uint32), host(d[1], np.uint32), host(d[2], np.float32))
    assert_matrix(got, ga.ani_matrix_groups_host(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS, k=K))
    assert sorted(summary) == MATRIX_KEYS

    runs = ctx.synth_device(2, 64, 2, 0.01, 1, dev(np.zeros(8, np.uint32)).view(torch.int32))
    assert runs.dtype == ga.RUN_DTYPE and runs["len"].tolist() == [64, 64] and runs["base"].tolist() == [0, 64]
    runs = ctx.synth_mixed_device(np.array([64, 64], np.uint32), 2, 0.01, 0.0, 1,
                                  dev(np.zeros(8, np.uint32)).view(torch.int32))
    assert runs.dtype == ga.RUN_DTYPE and runs["len"].tolist() == [64, 64]


def test_device_queries_and_explicit_stream(env):
    e, ctx, torch = env, env.ctx, torch_dev()
    q_sk, q_lens = e.sk[:1], e.lens[:1]
    exp = ga.query_host(e.sk, e.lens, q_sk, q_lens, MIN_ANI, k=K)
    exp_ani = pair_ani(exp)
    d_q, d_qlen = dev(q_sk), dev(q_lens)

    def outputs():
        return dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64))

    def found(d_out, d_count):
        n = int(host(d_count, np.uint64)[0])
        got = host(d_out, ga.PAIR_DTYPE)[:n]
        return got[np.lexsort((got["j"], got["i"]))]

    d_out, d_count = outputs()
    refused(INVALID, "min_ani is NaN", ctx.query_rows_device, e.d_sk, e.d_lens, N, d_q, d_qlen, 1, NAN, d_out, 4, d_count)
    assert ctx.query_rows_device(e.d_sk, e.d_lens, N, d_q, d_qlen, 1, MIN_ANI, d_out, 4, d_count) is None
    torch.cuda.synchronize()
    by_tensors = found(d_out, d_count)
    assert same_pairs(by_tensors, exp)

    d_best, d_best_ani = dev(np.zeros(1, ga.PAIR_DTYPE)), dev(np.zeros(1, np.float32))
    assert ctx.query_best_device(N, 1, dev(exp), dev(exp_ani), len(exp), None, d_best, d_best_ani) is None
    torch.cuda.synchronize()
    exp_best, exp_best_ani = ga.query_best_host(N, 1, exp, exp_ani)
    assert same_pairs(host(d_best, ga.PAIR_DTYPE), exp_best)
    assert f32_bits(host(d_best_ani, np.float32)) == f32_bits(exp_best_ani)

    # integer pointers and a stream of the caller's: the same result
    stream = torch.cuda.Stream()
    d_out, d_count = outputs()
    torch.cuda.synchronize()
    ctx.query_rows_device(e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, d_q.data_ptr(), d_qlen.data_ptr(), 1, MIN_ANI,
                          d_out.data_ptr(), 4, d_count.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert found(d_out, d_count).tolist() == by_tensors.tolist()

    d_out, d_count = outputs()
    torch.cuda.synchronize()
    ctx.pairs_device(e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, 0, ga.pair_tiles(N), MIN_ANI, d_out.data_ptr(), 4,
                     d_count.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert same_pairs(found(d_out, d_count), e.exp)


# ---- the galah port: the pairs path around a call, the finch wrap ------------------------------
def test_preclusterer_pairs_path(env, monkeypatch):
    e, ctx = env, env.ctx
    monkeypatch.setattr(ga, "_context", lambda k, s: ctx)
    calls = []
    real = ctx.set_pairs_path

    def recorded(path):
        calls.append(path)
        return real(path)

    monkeypatch.setattr(ctx, "set_pairs_path", recorded)
    routed = ["matrix", "auto"] if ctx.device_count == 1 else []  # (ignored on several devices)
    ctx.set_pairs_path("auto")  # what was set before is put back, not "default"
    try:
        pre = ga.FinchPreclusterer(MIN_ANI, num_kmers=S, kmer_length=K, pairs_path="matrix")
        clu = ga.FinchClusterer(MIN_ANI, num_kmers=S, kmer_length=K)
        want = {(0, 1): e.fexp_ani[0]}
        failed = "Failed to sketch genomes with finch: %s (status 2)" % e.io_message

        def after(expected_calls):
            assert ctx.pairs_path == "auto" and calls == expected_calls
            del calls[:]

        del calls[:]
        assert pre.distances(e.paths).internal == want
        after(routed)
        state = pre.distances_state(e.paths)
        assert state.cache().internal == want and state.paths == e.paths
        after(routed)
        state = pre.update(pre.distances_state(e.paths[:2]), e.paths[2:])
        assert state.cache().internal == want
        after(routed * 2)
        assert ga.cluster(e.paths, pre, clu) == [[0, 1], [2]]
        after(routed)
        with pre.collection() as col:
            assert col.add(e.paths) == 1 and col.cache().internal == want
            after(routed)
            assert col.cluster(clu) == [[0, 1], [2]]
            after([])
            with pytest.raises(RuntimeError) as x:
                col.add([e.missing[0]])
            assert type(x.value) is RuntimeError and str(x.value) == failed
            assert type(x.value.__cause__) is ga.GalahGpuError and x.value.__cause__.status == IO
            assert col.paths == e.paths
            after(routed)

        for failing in (lambda: pre.distances(e.bad_paths), lambda: pre.update(state, [e.missing[0]]),
                        lambda: ga.cluster(e.bad_paths, pre, clu)):
            with pytest.raises(RuntimeError) as x:
                failing()
            assert type(x.value) is RuntimeError and str(x.value) == failed
            assert type(x.value.__cause__) is ga.GalahGpuError
            after(routed)
    finally:
        real("default")


# ---- the call of bench.py's timed step ------------------------------------------------------------
def test_precluster_shards(env):
    e, ctx, torch = env, env.ctx, torch_dev()
    # one shard per member: all three genomes, or genomes 0 and 1 | genome 2
    shards = []
    for seqs in ([e.seqs] if ctx.device_count == 1 else [e.seqs[:2], e.seqs[2:]]):
        pk = ga.pack_records([[s] for s in seqs], k=K)
        shards.append((dev(pk.words).view(torch.int32), pk.runs.copy(), len(seqs)))
    value_error("one shard per device", ctx.precluster_shards, shards + shards[:1], MIN_ANI)
    value_error("one shard per device", ctx.precluster_shards, [], MIN_ANI)
    refused(INVALID, "min_ani is NaN", ctx.precluster_shards, shards, NAN)
    pairs, ani = ctx.precluster_shards(shards, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    assert shapes(pairs, ani) == [(ga.PAIR_DTYPE, (1,)), (np.dtype(np.float32), (1,))]
    pairs, ani = ctx.precluster_shards([(s[0], ga.device_runs(s[1], "cuda"), s[2]) for s in shards], MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)  # (the run table on the device)
    # no genome in any shard: nothing is sketched, no pair
    none = [(dev(np.zeros(1, np.uint32)).view(torch.int32), np.zeros(0, ga.RUN_DTYPE), 0)] * ctx.device_count
    assert shapes(*ctx.precluster_shards(none, MIN_ANI)) == [PAIRS0, F32_0]


# ---- n == 0 of the calls that do not return before their device code ---------------------------------
def test_no_input(env):
    """No paths, no rows, no pairs, no queries: ordinary calls; dtype and shape of every value returned."""
    e, ctx = env, env.ctx
    ctx.last_cached = 7
    assert shapes(*ctx.precluster_files([], MIN_ANI)) == [PAIRS0, F32_0] and ctx.last_cached == 0
    blocks = []
    ctx.last_cached = 7
    assert shapes(*ctx.precluster_files_each([], MIN_ANI, blocks.append)) == [PAIRS0, F32_0]
    assert blocks == [] and ctx.last_cached == 0
    assert shapes(*ctx.precluster_files(e.paths[:1], MIN_ANI)) == [PAIRS0, F32_0]  # (one file: no pair to compare)

    rep, pairs, ani = ctx.cluster_files([], MIN_ANI, MIN_ANI)
    assert shapes(rep, pairs, ani) == [U32_0, PAIRS0, F32_0]
    rep = ctx.cluster_files([], MIN_ANI, MIN_ANI, want_pairs=False)
    assert type(rep) is np.ndarray and shapes(rep) == [U32_0]

    for v in (ctx.validate_files([], [], MIN_ANI), ctx.validate_clusters(EMPTY_SK, EMPTY_LENS, [], MIN_ANI),
              ctx.validate_clusters(e.sk, e.lens, [], MIN_ANI)):
        assert type(v) is ga.Validation and v.ok and shapes(v.bad, v.bad_ani) == [PAIRS0, F32_0]
        assert (v.member_pairs, v.member_bad, v.rep_pairs, v.rep_bad) == (0, 0, 0, 0)

    keys = sorted(f for f, _ in ga._PairsMatrixSummary._fields_)
    for pairs, summary in (ctx.pairs_matrix(EMPTY_SK, EMPTY_LENS, MIN_ANI), ctx.pairs_matrix(e.sk, e.lens, MIN_ANI, rows=[]),
                           ctx.pairs_border_matrix(EMPTY_SK, EMPTY_LENS, 0, MIN_ANI),
                           ctx.pairs_border_matrix(e.sk, e.lens, N, MIN_ANI)):
        assert shapes(pairs) == [PAIRS0] and sorted(summary) == keys
        assert summary["n_pairs"] == 0 and summary["path"] == "matrix"  # (no pair: nothing is run, the path is named)

    members, offsets, local, poff = ctx.preclusters(0, np.zeros(0, ga.PAIR_DTYPE))
    assert shapes(members, local) == [U32_0, (ga.LOCAL_PAIR_DTYPE, (0,))]
    assert offsets.dtype == np.uint32 and offsets.tolist() == [0] and poff.dtype == np.uint64 and poff.tolist() == [0]
    members, offsets, local, poff = ctx.preclusters(0, np.zeros(0, ga.PAIR_DTYPE), with_pairs=False)
    assert shapes(members) == [U32_0] and offsets.tolist() == [0] and local is None and poff is None
    members, offsets, local, poff = ctx.preclusters(N, np.zeros(0, ga.PAIR_DTYPE))  # no pair: every genome its own set
    assert members.tolist() == [0, 1, 2] and offsets.tolist() == [0, 1, 2, 3] and poff.tolist() == [0, 0, 0, 0]
    assert shapes(local) == [(ga.LOCAL_PAIR_DTYPE, (0,))]

    h = ctx.collection_load(EMPTY_SK, EMPTY_LENS, np.zeros(0, ga.PAIR_DTYPE), np.zeros(0, np.float32), MIN_ANI)
    try:
        assert type(h) is int and ctx.collection_stat(h)[0]["n_rows"] == 0
        assert shapes(*ctx.collection_rows(h)) == ROWS0
        assert shapes(ctx.collection_remove(h, [])) == [U32_0]
        assert shapes(*ctx.collection_query_rows(h, EMPTY_SK, EMPTY_LENS, MIN_ANI)) == [PAIRS0, F32_0]
    finally:
        ctx.collection_destroy(h)
    with Col(e) as col:
        new_index = ctx.collection_remove(col.h, [])  # no row named: every row keeps its index
        assert new_index.dtype == np.uint32 and new_index.tolist() == [0, 1, 2]
        assert shapes(*ctx.collection_query_rows(col.h, EMPTY_SK, EMPTY_LENS, MIN_ANI)) == [PAIRS0, F32_0]
        col.assert_unchanged()


# ---- class Collection: its own checks' texts, and the methods above the context's ---------------------
def test_collection_class(env, monkeypatch):
    e, ctx = env, env.ctx
    monkeypatch.setattr(ga, "_context", lambda k, s: ctx)
    pre = ga.FinchPreclusterer(MIN_ANI, num_kmers=S, kmer_length=K)
    clu = ga.FinchClusterer(MIN_ANI, num_kmers=S, kmer_length=K)

    class Other(ga.FinchClusterer):
        def method_name(self):
            return "skani"

    with pre.collection() as col:
        assert col.add(e.paths[:2]) == 1 and col.add(e.paths[2:]) == 0 and len(col) == N and col.paths == e.paths
        value_error("genome already present: " + e.paths[1], col.add, [e.paths[1]])
        value_error("genome already present: new.fna", col.add, ["new.fna", "new.fna"])
        value_error("genome not present: new.fna", col.remove, ["new.fna"])
        info = col.info()
        assert info["n_rows"] == N and info["n_pairs"] == 1
        for order in ([0, 1], [0, 1, 1], [0, 1, 3]):
            value_error("order must be a permutation of 0 .. 2", col.cluster, clu, order)
            value_error("order must be a permutation of 0 .. 2", col.classify, e.paths[:1], clu, order)
        for name, call in (("cluster", lambda: col.cluster(Other(MIN_ANI))),
                           ("classify", lambda: col.classify(e.paths[:1], Other(MIN_ANI)))):
            with pytest.raises(NotImplementedError) as x:
                call()
            assert str(x.value) == "galah_amd.Collection.%s: only finch + finch runs here, not finch + skani" % name
        assert col.cluster(clu) == [[0, 1], [2]] and col.cluster(clu, order=[2, 1, 0]) == [[0], [1, 2]]
        # asked again, each file finds itself (ANI 1.0) and its neighbour; it joins its representative
        hits = col.query(e.paths[:1])
        assert [[i for i, _ in h] for h in hits] == [[0, 1]] and hits[0][0][1] == np.float32(1.0)
        assert type(hits[0][1][1]) is np.float32 and hits[0][1][1] == e.fexp_ani[0]
        assert col.query([]) == [] and col.classify([], clu) == []
        got = col.classify([e.paths[1], e.paths[2]], clu)
        assert got == [(0, e.fexp_ani[0]), (2, np.float32(1.0))]

        state = col.state()
        assert type(state) is ga.PreclusterState and state.paths == e.paths and state.cache().internal == col.cache().internal
        assert same_pairs(state.pairs, e.fexp) and (state.lens == e.flens).all()
        other = ga.FinchPreclusterer(MIN_ANI, num_kmers=S, kmer_length=K - 1)
        value_error("PreclusterState of k=%d s=%d seed=%d min_ani=%r, preclusterer of k=%d s=%d seed=0 min_ani=%r"
                    % (K, S, 0, state.min_ani, K - 1, S, other.min_ani), ga.Collection.from_state, state, other)
        value_error("PreclusterState of k=%d s=%d seed=%d min_ani=%r, preclusterer of k=%d s=%d seed=0 min_ani=%r"
                    % (K, S, 0, state.min_ani, K - 1, S, other.min_ani), other.update, state, [])
        with ga.Collection.from_state(state, pre) as again:
            assert again.paths == e.paths and again.cache().internal == col.cache().internal
            assert again.cluster(clu) == [[0, 1], [2]]
        col.remove(e.paths[2:])
        assert col.paths == e.paths[:2] and col.info()["n_rows"] == 2 and col.cluster(clu) == [[0, 1]]

    with pytest.raises(NotImplementedError) as x:
        ga.cluster_update(state, [], pre, Other(MIN_ANI))
    assert str(x.value) == "galah_amd.cluster_update: only finch + finch runs here, not finch + skani"
    value_error("order must be a permutation of 0 .. 2", ga.relabel_pairs, e.fexp, [0, 1, 1])
