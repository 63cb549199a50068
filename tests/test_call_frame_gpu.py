"""The failure paths at the C ABI, pinned before the host call frame moved
("the host call frame").  Needs an MI355X.

One case per extern "C" entry point that takes a gg_ctx* or a gg_collection*
and can fail on its arguments, each on a one-device context and on the
two-member context over one device ([0, 0]) on which primary(ctx) != ctx, so
that the message has to travel from the first member to the context given.

Every status and every message in the table was read from the library's source
as it stood before the call frame was shared (commit 0fe1447: the fail() and
check_*() calls of galah_amd/csrc/*.cpp and *.hip); nothing was taken from what
a run printed.  The same holds for the state of the outputs: "kept" where that
source refuses the argument before it resets the outputs, reset where it
resets them first.  The table is the contract: the same file passes on a
library built from that commit (GALAHGPU_LIB) and on this tree's.

A case asserts
  - the status code;
  - the exact text of gg_last_error on the context that was passed;
  - the state of every output (lists, counts, summaries, n_border);
  - that a small valid call of the same entry point on the same context
    succeeds straight afterwards and equals the host form where one exists.

No case asks the device to fault: each is refused by a host check before any
launch, or is an ordinary file error.
"""
import ctypes
import os

import numpy as np
import pytest

import galah_amd as ga
import oracle
from test_pair_edges import quads, torch_dev

pytestmark = pytest.mark.gpu

L = ga.lib()
F, byref = ctypes.c_float, ctypes.byref
vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
INVALID, IO, CANCELLED = 1, 2, 9
K, S, N = 21, 32, 3
NAN = float("nan")
MIN_ANI = float(np.float32(0.9))
POISON = 0x10  # a caller's value in an output pointer: never freed, never followed
CONTEXTS = {"one": [0], "two": [0, 0]}


def ptr(a):
    return a.ctypes.data_as(vp)


def dev(a):
    """The bytes of a numpy array in device memory (a u8 tensor)."""
    torch = torch_dev()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def paths_arg(paths):
    return (ctypes.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])


def same_pairs(got, exp):
    return quads(got).tolist() == quads(exp).tolist()


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def pair_ani(p):
    return np.array([ga.ani_f32(int(c), int(t), K) for c, t in zip(p["common"], p["total"])], np.float32)


def is_zero(struct):
    return bytes(struct) == bytes(ctypes.sizeof(struct))


def fill(struct):
    ctypes.memset(byref(struct), 0x5A, ctypes.sizeof(struct))
    return struct


class Env:
    """What the cases share on one context: 3 rows x 32 slots (rows 0 and 1
    share 30 hashes, row 2 holds 20 of its own), the same rows on the device,
    three FASTA files of 400 bases (the second a copy of the first with three
    substitutions) and the host forms' answers over both."""

    def __init__(self, devices, tmp):
        self.ctx = ga.Context(k=K, sketch_size=S, devices=devices)
        self.c = self.ctx._c
        rng = np.random.default_rng(7)
        pool = np.sort(rng.choice(1 << 40, size=S + 2 + 20, replace=False).astype(np.uint64))
        self.sk = np.zeros((N, S), np.uint64)
        self.sk[0] = pool[:S]
        self.sk[1] = np.sort(np.concatenate([pool[:S - 2], pool[S:S + 2]]))
        self.sk[2, :20] = pool[S + 2:]
        self.lens = np.array([S, S, 20], np.uint32)
        self.long_lens = np.array([S, S + 1, 20], np.uint32)
        self.exp = ga.pairs_border_host(self.sk, self.lens, 0, MIN_ANI, k=K)  # (n_old = 0: gg_pairs' set)
        assert quads(self.exp)[:, :2].tolist() == [[0, 1]]
        self.exp_ani = pair_ani(self.exp)
        self.d_sk, self.d_lens = dev(self.sk), dev(self.lens)
        # files
        bases = np.frombuffer(b"ACGT", np.uint8)
        g0 = bases[rng.integers(0, 4, 400)]
        g1 = g0.copy()
        for at in (50, 200, 350):
            g1[at] = bases[(int(np.where(bases == g1[at])[0][0]) + 1) % 4]
        g2 = bases[rng.integers(0, 4, 400)]
        self.seqs = [g.tobytes() for g in (g0, g1, g2)]
        self.paths = []
        for x, seq in enumerate(self.seqs):
            p = os.path.join(tmp, "g%d.fna" % x)
            with open(p, "wb") as f:
                f.write(b">g%d\n" % x + seq + b"\n")
            self.paths.append(p)
        self.missing = [os.path.join(tmp, "missing_a.fna"), os.path.join(tmp, "missing_b.fna")]
        self.bad_paths = [self.paths[0], self.missing[0], self.paths[1], self.missing[1]]
        self.io_message = "could not open " + self.missing[0]
        self.fsk = np.zeros((N, S), np.uint64)
        self.flens = np.zeros(N, np.uint32)
        for x, seq in enumerate(self.seqs):
            h = oracle.sketch_sequence(seq, K, S)
            self.fsk[x, :len(h)] = h
            self.flens[x] = len(h)
        self.fexp = ga.pairs_border_host(self.fsk, self.flens, 0, MIN_ANI, k=K)
        assert quads(self.fexp)[:, :2].tolist() == [[0, 1]]
        self.fexp_ani = pair_ani(self.fexp)

    def error(self):
        return L.gg_last_error(self.c).decode()

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=sorted(CONTEXTS))
def env(request, tmp_path_factory):
    e = Env(CONTEXTS[request.param], str(tmp_path_factory.mktemp("call_frame")))
    yield e
    e.close()


# ----------------------------------------------------------------------------
# The table.  A case is a generator: it makes the failing call and yields its
# status (the runner then reads gg_last_error at once), goes on to assert the
# outputs and ends with the valid call.  message: a string, or a function of
# the Env (a path in it).
# ----------------------------------------------------------------------------
CASES = []


def case(name, status, message):
    def deco(fn):
        CASES.append(pytest.param(fn, status, message, id=name))
        return fn
    return deco


def assert_rows_from_files(e, sk, lens):
    assert lens.tolist() == e.flens.tolist()
    for g in range(N):
        assert (sk[g, :lens[g]] == e.fsk[g, :lens[g]]).all()


# ---- api.cpp ----------------------------------------------------------------
@case("gg_sketch_device", INVALID, "gg_sketch_device: null buffer")
def _(e):
    yield L.gg_sketch_device(e.c, None, 0, None, 1, 1, None, None, None)
    pk = ga.pack_records([[s] for s in e.seqs], k=K)
    d_words = dev(pk.words).view(torch_dev().int32)
    d_out, d_len = dev(np.zeros((N, S), np.uint64)), dev(np.zeros(N, np.uint32))
    e.ctx.sketch_device(d_words, pk.runs.copy(), N, d_out, d_len)
    assert_rows_from_files(e, host(d_out, np.uint64).reshape(N, S), host(d_len, np.uint32))


@case("gg_pairs_device", INVALID, "gg_pairs_device: null buffer")
def _(e):
    yield L.gg_pairs_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, 0, 1, F(MIN_ANI), None, 0, None, None)
    d_out, d_count = dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64))
    e.ctx.pairs_device(e.d_sk, e.d_lens, N, 0, ga.pair_tiles(N), MIN_ANI, d_out, 4, d_count)
    torch_dev().cuda.synchronize()
    assert host(d_count, np.uint64)[0] == 1 and same_pairs(host(d_out, ga.PAIR_DTYPE)[:1], e.exp)


@case("gg_timing_read", INVALID, "gg_timing_read: bad argument")
def _(e):
    k = ga._KStats()
    yield L.gg_timing_read(e.c, -1, byref(k))
    assert e.ctx.timing_read(ga.KERNEL_PAIRS)["launches"] == 0


@case("gg_synth_clustered_device", INVALID, "gg_synth_clustered_device: bad arguments")
def _(e):
    runs = np.zeros(2, ga.RUN_DTYPE)
    d_words = dev(np.zeros(8, np.uint32))
    yield L.gg_synth_clustered_device(e.c, 0, 2, 63, 2, F(0.01), 1, d_words.data_ptr(), ptr(runs), None)
    runs = e.ctx.synth_device(2, 64, 2, 0.01, 1, d_words.view(torch_dev().int32))
    assert runs["len"].tolist() == [64, 64] and runs["base"].tolist() == [0, 64]


@case("gg_synth_mixed_device", INVALID, "gg_synth_mixed_device: bad arguments")
def _(e):
    lens, runs, nr = np.array([64, 64], np.uint32), np.zeros(8, ga.RUN_DTYPE), u64(7)
    d_words = dev(np.zeros(8, np.uint32))
    yield L.gg_synth_mixed_device(e.c, 0, 2, ptr(lens), 0, F(0.01), ctypes.c_double(0.0), 1, d_words.data_ptr(),
                                  ptr(runs), 8, byref(nr), None)
    assert nr.value == 7  # kept
    runs = e.ctx.synth_mixed_device(lens, 2, 0.01, 0.0, 1, d_words.view(torch_dev().int32))
    assert runs["len"].tolist() == [64, 64]


@pytest.mark.parametrize("name, call", [
    ("gg_phase_times", lambda e: L.gg_phase_times(e.c, None)),
    ("gg_pair_paths", lambda e: L.gg_pair_paths(e.c, None)),
    ("gg_fallbacks", lambda e: L.gg_fallbacks(e.c, None)),
    ("gg_peer_links", lambda e: L.gg_peer_links(e.c, None)),
    ("gg_info_line", lambda e: L.gg_info_line(e.c, None, 16)),
])
def test_null_argument_on_the_thread(env, name, call):
    """The read-outs: a null output is reported on the calling thread (they take a const context)."""
    L.gg_set_pairs_path(env.c, 99)
    before = env.error()
    assert call(env) == INVALID
    assert L.gg_thread_last_error().decode() == name + ": null argument"
    assert env.error() == before == "gg_set_pairs_path: unknown path"
    assert sorted(env.ctx.phase_times()) == sorted(ga.PHASES) and len(env.ctx.pair_paths()) == 5
    assert len(env.ctx.fallbacks()) == len(ga.FALLBACKS) and env.ctx.info_line().startswith("galahgpu: ")
    assert env.ctx.peer_links().shape == (env.ctx.device_count,) * 2


# ---- multi.cpp ----------------------------------------------------------------
@case("gg_sketch", INVALID, "gg_sketch: null buffer")
def _(e):
    yield L.gg_sketch(e.c, None, None, None)
    sk, lens = e.ctx.sketch(ga.pack_records([[s] for s in e.seqs], k=K))
    assert_rows_from_files(e, sk, lens)


@case("gg_pairs", INVALID, "sketch longer than sketch_size")
def _(e):
    out, n = vp(POISON), u64(7)
    yield L.gg_pairs(e.c, ptr(e.sk), ptr(e.long_lens), N, F(MIN_ANI), byref(out), byref(n))
    assert out.value is None and n.value == 0
    assert same_pairs(e.ctx.pairs(e.sk, e.lens, MIN_ANI), e.exp)


@case("gg_sketch_files", INVALID, "gg_sketch_files: null argument")
def _(e):
    hits = u32(7)
    yield L.gg_sketch_files(e.c, paths_arg(e.paths), N, None, None, None, byref(hits))
    assert hits.value == 7  # kept
    sk, lens, _ = e.ctx.sketch_files(e.paths)
    assert_rows_from_files(e, sk, lens)


@case("gg_sketch_files_stats", INVALID, "gg_sketch_files_stats: null argument")
def _(e):
    sk, lens = np.zeros((N, S), np.uint64), np.zeros(N, np.uint32)
    yield L.gg_sketch_files_stats(e.c, paths_arg(e.paths), N, None, ptr(sk), ptr(lens), None)
    sk, lens, stats = e.ctx.sketch_files_stats(e.paths)
    assert_rows_from_files(e, sk, lens)
    assert stats == [ga.calculate_genome_stats(p) for p in e.paths]


def files_call(e, name, paths, min_ani, extra=()):
    """gg_precluster_files_cached / _resident: (status, pairs, ani, n_out) with the outputs poisoned."""
    pp, ap, n = vp(POISON), vp(POISON), u64(7)
    st = getattr(L, name)(e.c, paths_arg(paths), len(paths), F(min_ani), None, byref(pp), byref(ap), byref(n), *extra)
    return st, pp, ap, n


@case("gg_precluster_files_cached", INVALID, "min_ani is NaN")
def _(e):
    hits = u32(7)
    st, pp, ap, n = files_call(e, "gg_precluster_files_cached", e.paths, NAN, (byref(hits),))
    yield st
    assert (pp.value, ap.value, n.value, hits.value) == (POISON, POISON, 7, 7)  # kept
    pairs, ani = e.ctx.precluster_files(e.paths, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)


@case("gg_precluster_files", INVALID, "min_ani is NaN")
def _(e):
    pp, ap, n = vp(POISON), vp(POISON), u64(7)
    yield L.gg_precluster_files(e.c, paths_arg(e.paths), N, F(NAN), byref(pp), byref(ap), byref(n))
    assert (pp.value, ap.value, n.value) == (POISON, POISON, 7)  # kept
    pp, ap, n = vp(), vp(), u64()
    assert L.gg_precluster_files(e.c, paths_arg(e.paths), N, F(MIN_ANI), byref(pp), byref(ap), byref(n)) == 0
    pairs, ani = e.ctx._pairs_ani(pp, ap, n.value)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)


def each_call(e, paths, min_ani, sink):
    pp, ap, n, hits = vp(POISON), vp(POISON), u64(7), u32(7)
    cb = ga.PAIR_SINK(sink) if sink else ctypes.cast(None, ga.PAIR_SINK)
    st = L.gg_precluster_files_each(e.c, paths_arg(paths), len(paths), F(min_ani), None, cb, None, byref(pp), byref(ap),
                                    byref(n), byref(hits))
    return st, pp, ap, n, hits


def assert_each(e):
    blocks = []
    pairs, ani = e.ctx.precluster_files_each(e.paths, MIN_ANI, lambda blk: blocks.append(blk.copy()) and False)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    every = ga.pairs_border_host(e.fsk, e.flens, 0, 0.0, k=K)
    assert len(every) == 3 and same_pairs(np.concatenate(blocks), every)


@case("gg_precluster_files_each", INVALID, "gg_precluster_files_each: null argument")
def _(e):
    st, pp, ap, n, hits = each_call(e, e.paths, MIN_ANI, None)
    yield st
    assert (pp.value, ap.value, n.value, hits.value) == (POISON, POISON, 7, 7)  # kept
    assert_each(e)


@case("gg_precluster_files_each_io", IO, lambda e: e.io_message)
def _(e):
    st, pp, ap, n, hits = each_call(e, e.bad_paths, MIN_ANI, lambda user, p, cnt: 0)
    yield st
    assert (pp.value, ap.value, n.value, hits.value) == (None, None, 0, 0)
    assert_each(e)


@case("gg_precluster_files_each_cancelled", CANCELLED, "gg_precluster_files_each: the pair sink stopped the call")
def _(e):
    st, pp, ap, n, hits = each_call(e, e.paths, MIN_ANI, lambda user, p, cnt: 1)
    yield st
    assert (pp.value, ap.value, n.value, hits.value) == (None, None, 0, 0)
    assert_each(e)


def assert_cluster_summary(e, summary):
    # (a multi-device context takes gg_cluster_files' path: ani_rechecked and pair_passes are 0 there)
    assert summary["n_pairs"] == 1 and summary["n_preclusters"] == 2 and summary["largest_precluster"] == 2
    assert summary["pair_passes"] == (1 if e.ctx.device_count == 1 else 0)


def cluster_resident_call(e, paths, min_ani, cluster_ani):
    rep, summary = np.full(max(len(paths), 1), 7, np.uint32), fill(ga._ClusterSummary())
    st = L.gg_cluster_files_resident(e.c, paths_arg(paths), len(paths), F(min_ani), F(cluster_ani), None, ptr(rep),
                                     byref(summary))
    return st, rep, summary


def assert_cluster_resident(e):
    rep, summary = e.ctx.cluster_files_resident(e.paths, MIN_ANI, MIN_ANI)
    assert rep.tolist() == ga.cluster_pairs_host(N, e.fexp, e.fexp_ani, MIN_ANI).tolist() == [0, 0, 2]
    assert_cluster_summary(e, summary)


@case("gg_cluster_files_resident", INVALID, "gg_cluster_files_resident: min_ani or cluster_ani is NaN")
def _(e):
    st, rep, summary = cluster_resident_call(e, e.paths, MIN_ANI, NAN)
    yield st
    assert is_zero(summary) and rep.tolist() == [7, 7, 7]
    assert_cluster_resident(e)


@case("gg_cluster_files_resident_io", IO, lambda e: e.io_message)
def _(e):
    st, rep, summary = cluster_resident_call(e, e.bad_paths, MIN_ANI, MIN_ANI)
    yield st
    assert is_zero(summary)
    assert_cluster_resident(e)


@case("gg_precluster_files_resident", INVALID, "gg_precluster_files_resident: min_ani is NaN")
def _(e):
    summary = fill(ga._PairsMatrixSummary())
    st, pp, ap, n = files_call(e, "gg_precluster_files_resident", e.paths, NAN, (byref(summary),))
    yield st
    assert (pp.value, ap.value, n.value) == (POISON, POISON, 7) and is_zero(summary)  # the lists kept, the summary cleared
    pairs, ani, summary = e.ctx.precluster_files_resident(e.paths, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)
    assert summary["n_pairs"] == 1 and summary["path"] == "default" and summary["pair_passes"] == 1


@case("gg_precluster_files_resident_io", IO, lambda e: e.io_message)
def _(e):
    summary = fill(ga._PairsMatrixSummary())
    st, pp, ap, n = files_call(e, "gg_precluster_files_resident", e.bad_paths, MIN_ANI, (byref(summary),))
    yield st
    assert (pp.value, ap.value, n.value) == (None, None, 0) and is_zero(summary)
    pairs, ani, _ = e.ctx.precluster_files_resident(e.paths, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)


def matrices_call(e, paths, min_ani, want=True):
    outs = [vp(POISON) for _ in range(6)]  # members, offsets, cell_offsets, common, total, ani
    ng, summary = u32(7), fill(ga._MatrixSummary())
    st = L.gg_precluster_matrices_files(e.c, paths_arg(paths), len(paths), F(min_ani), None, byref(outs[0]),
                                        byref(outs[1]), byref(ng), byref(outs[2]),
                                        *[byref(o) if want else None for o in outs[3:]], byref(summary))
    return st, [o.value for o in outs], ng.value, summary


def assert_matrices(e):
    members, offsets, cells, common, total, ani, _ = e.ctx.precluster_matrices_files(e.paths, MIN_ANI)
    assert members.tolist() == [0, 1, 2] and offsets.tolist() == [0, 2, 3] and cells.tolist() == [0, 4, 5]
    c, t, a = ga.ani_matrix_groups_host(e.fsk, e.flens, members, offsets, k=K)[:3]
    assert common.tolist() == c.tolist() and total.tolist() == t.tolist() and f32_bits(ani) == f32_bits(a)


@case("gg_precluster_matrices_files", INVALID, "gg_precluster_matrices_files: min_ani is NaN")
def _(e):
    st, outs, ng, summary = matrices_call(e, e.paths, NAN)
    yield st
    assert outs == [POISON] * 6 and ng == 7 and is_zero(summary)  # the arrays kept, the summary cleared
    assert_matrices(e)


@case("gg_precluster_matrices_files_io", IO, lambda e: e.io_message)
def _(e):
    st, outs, ng, summary = matrices_call(e, e.bad_paths, MIN_ANI)
    yield st
    assert outs == [None] * 6 and ng == 0 and is_zero(summary)
    assert_matrices(e)


@case("gg_precluster_shards", INVALID, "gg_precluster_shards: null argument")
def _(e):
    pp, ap, n = vp(POISON), vp(POISON), u64(7)
    yield L.gg_precluster_shards(e.c, None, F(MIN_ANI), byref(pp), byref(ap), byref(n))
    assert (pp.value, ap.value, n.value) == (POISON, POISON, 7)  # kept
    # one shard per member: all three genomes, or genomes 0 and 1 | genome 2
    shards = []
    for seqs in ([e.seqs] if e.ctx.device_count == 1 else [e.seqs[:2], e.seqs[2:]]):
        pk = ga.pack_records([[s] for s in seqs], k=K)
        shards.append((dev(pk.words).view(torch_dev().int32), pk.runs.copy(), len(seqs)))
    pairs, ani = e.ctx.precluster_shards(shards, MIN_ANI)
    assert same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)


# ---- border.cpp ---------------------------------------------------------------
@case("gg_pairs_border", INVALID, "sketch longer than sketch_size")
def _(e):
    out, n = vp(POISON), u64(7)
    yield L.gg_pairs_border(e.c, ptr(e.sk), ptr(e.long_lens), N, 1, F(MIN_ANI), byref(out), byref(n))
    assert out.value is None and n.value == 0
    assert same_pairs(e.ctx.pairs_border(e.sk, e.lens, 1, MIN_ANI), e.exp)


@case("gg_pairs_border_device", INVALID, "gg_pairs_border_device: n_old exceeds n")
def _(e):
    d_out, d_count = dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64))
    yield L.gg_pairs_border_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, N + 1, F(MIN_ANI), d_out.data_ptr(),
                                   4, d_count.data_ptr(), None)
    assert host(d_count, np.uint64)[0] == 0
    e.ctx.pairs_border_device(e.d_sk, e.d_lens, N, 1, MIN_ANI, d_out, 4, d_count)
    torch_dev().cuda.synchronize()
    assert host(d_count, np.uint64)[0] == 1 and same_pairs(host(d_out, ga.PAIR_DTYPE)[:1], e.exp)


@case("gg_update_files", INVALID, "sketch longer than sketch_size")
def _(e):
    new_sk, new_lens = np.zeros((1, S), np.uint64), np.zeros(1, np.uint32)
    pp, ap, n = vp(POISON), vp(POISON), u64(7)
    old_lens = np.array([S + 1, e.flens[1]], np.uint32)
    yield L.gg_update_files(e.c, ptr(e.fsk), ptr(old_lens), 2, paths_arg(e.paths[2:]), 1, F(MIN_ANI), None, ptr(new_sk),
                            ptr(new_lens), byref(pp), byref(ap), byref(n))
    assert (pp.value, ap.value, n.value) == (None, None, 0)
    # rows 0 and 2 old, the file of row 1 new: the border is the pair of rows 0 and 1 as (0, 2)
    old_sk, old_lens = e.fsk[[0, 2]], e.flens[[0, 2]]
    new_sk, new_lens, pairs, ani = e.ctx.update_files(old_sk, old_lens, e.paths[1:2], MIN_ANI)
    assert (new_sk[0] == e.fsk[1]).all() and new_lens.tolist() == [e.flens[1]]
    exp = ga.pairs_border_host(e.fsk[[0, 2, 1]], e.flens[[0, 2, 1]], 2, MIN_ANI, k=K)
    assert quads(exp)[:, :2].tolist() == [[0, 2]] and same_pairs(pairs, exp) and f32_bits(ani) == f32_bits(pair_ani(exp))


# ---- cluster.hip, precluster.hip, ani_f32.hip ------------------------------------
def exp_rep(e):
    rep = ga.cluster_pairs_host(N, e.exp, e.exp_ani, MIN_ANI)
    assert rep.tolist() == [0, 0, 2]
    return rep


@case("gg_cluster_pairs", INVALID, "gg_cluster_pairs: cluster_ani is NaN")
def _(e):
    rep = np.full(N, 7, np.uint32)
    yield L.gg_cluster_pairs(e.c, N, ptr(e.exp), ptr(e.exp_ani), 1, F(NAN), ptr(rep))
    assert rep.tolist() == [7, 7, 7]
    assert e.ctx.cluster_pairs(N, e.exp, e.exp_ani, MIN_ANI).tolist() == exp_rep(e).tolist()


@case("gg_cluster_pairs_device", INVALID, "gg_cluster_pairs_device: cluster_ani is NaN")
def _(e):
    d_pairs, d_ani, d_rep = dev(e.exp), dev(e.exp_ani), dev(np.full(N, 7, np.uint32))
    yield L.gg_cluster_pairs_device(e.c, N, d_pairs.data_ptr(), d_ani.data_ptr(), 1, F(NAN), d_rep.data_ptr(), None)
    assert host(d_rep, np.uint32).tolist() == [7, 7, 7]
    e.ctx.cluster_pairs_device(N, d_pairs, d_ani, 1, MIN_ANI, d_rep)
    assert host(d_rep, np.uint32).tolist() == exp_rep(e).tolist()


@case("gg_cluster_files", INVALID, "gg_cluster_files: null rep_of or NaN cluster_ani")
def _(e):
    rep, pp, ap, n = np.full(N, 7, np.uint32), vp(POISON), vp(POISON), u64(7)
    yield L.gg_cluster_files(e.c, paths_arg(e.paths), N, F(MIN_ANI), F(NAN), None, ptr(rep), byref(pp), byref(ap),
                             byref(n))
    assert (pp.value, ap.value, n.value) == (None, None, 0) and rep.tolist() == [7, 7, 7]
    rep, pairs, ani = e.ctx.cluster_files(e.paths, MIN_ANI, MIN_ANI)
    assert rep.tolist() == [0, 0, 2] and same_pairs(pairs, e.fexp) and f32_bits(ani) == f32_bits(e.fexp_ani)


def exp_partition(e):
    members, offsets = ga.partition_preclusters(N, e.exp)
    assert members.tolist() == [0, 1, 2] and offsets.tolist() == [0, 2, 3]
    return members, offsets


@case("gg_preclusters", INVALID, "gg_preclusters: pair index out of range")
def _(e):
    bad = e.exp.copy()
    bad["i"] = N
    members, offsets, ns = np.full(N, 7, np.uint32), np.full(N + 1, 7, np.uint32), u32(7)
    yield L.gg_preclusters(e.c, N, ptr(bad), 1, ptr(members), ptr(offsets), byref(ns), None, None)
    assert ns.value == 7 and members.tolist() == [7] * N and offsets.tolist() == [7] * (N + 1)
    members, offsets, local, poff = e.ctx.preclusters(N, e.exp)
    em, eo = exp_partition(e)
    el, ep = ga.precluster_pairs(N, e.exp, em, eo)
    assert members.tolist() == em.tolist() and offsets.tolist() == eo.tolist()
    assert local.tolist() == el.tolist() and poff.tolist() == ep.tolist()


@case("gg_preclusters_device", INVALID, "gg_preclusters_device: null argument")
def _(e):
    d_pairs, d_members, d_offsets = dev(e.exp), dev(np.full(N, 7, np.uint32)), dev(np.full(N + 1, 7, np.uint32))
    ns = u32(7)
    yield L.gg_preclusters_device(e.c, N, d_pairs.data_ptr(), 1, d_members.data_ptr(), None, byref(ns), None, None, None)
    assert ns.value == 7 and host(d_members, np.uint32).tolist() == [7] * N
    assert e.ctx.preclusters_device(N, d_pairs, 1, d_members, d_offsets) == 2
    em, eo = exp_partition(e)
    assert host(d_members, np.uint32).tolist() == em.tolist() and host(d_offsets, np.uint32)[:3].tolist() == eo.tolist()


@case("gg_ani_f32_device", INVALID, "gg_ani_f32_device: null buffer")
def _(e):
    cnt = u64(7)
    yield L.gg_ani_f32_device(e.c, None, 1, None, None, byref(cnt), None)
    assert cnt.value == 0
    d_pairs, d_ani = dev(e.exp), dev(np.zeros(1, np.float32))
    e.ctx.ani_f32_device(d_pairs, 1, d_ani)
    assert f32_bits(host(d_ani, np.float32)) == f32_bits(e.exp_ani)


# ---- resident.cpp -------------------------------------------------------------
@case("gg_cluster_rows_device", INVALID, "gg_cluster_rows_device: min_ani or cluster_ani is NaN")
def _(e):
    d_rep, summary, pp, ap = dev(np.full(N, 7, np.uint32)), fill(ga._ClusterSummary()), vp(POISON), vp(POISON)
    yield L.gg_cluster_rows_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, F(NAN), F(MIN_ANI), d_rep.data_ptr(),
                                   byref(summary), byref(pp), byref(ap), None)
    assert is_zero(summary) and pp.value is None and ap.value is None and host(d_rep, np.uint32).tolist() == [7] * N
    summary, p, a, n_pairs = e.ctx.cluster_rows_device(e.d_sk, e.d_lens, N, MIN_ANI, MIN_ANI, d_rep)
    assert host(d_rep, np.uint32).tolist() == exp_rep(e).tolist() and n_pairs == 1 and p and a
    assert summary["n_preclusters"] == 2 and summary["largest_precluster"] == 2 and summary["pair_passes"] == 1


@case("gg_pairs_matrix_device", INVALID, "gg_pairs_matrix_device: min_ani is NaN")
def _(e):
    d_out, d_count, summary = dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64)), fill(ga._PairsMatrixSummary())
    yield L.gg_pairs_matrix_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, None, N, F(NAN), d_out.data_ptr(), 4,
                                   d_count.data_ptr(), byref(summary), None)
    assert is_zero(summary) and host(d_count, np.uint64)[0] == 0
    summary = e.ctx.pairs_matrix_device(e.d_sk, e.d_lens, N, None, N, MIN_ANI, d_out, 4, d_count)
    assert host(d_count, np.uint64)[0] == 1 and same_pairs(host(d_out, ga.PAIR_DTYPE)[:1], e.exp)
    assert summary["n_pairs"] == 1 and summary["path"] == "matrix"


@case("gg_pairs_matrix", INVALID, "gg_pairs_matrix: row index listed twice")
def _(e):
    rows, out, n, summary = np.array([0, 1, 1], np.uint32), vp(POISON), u64(7), fill(ga._PairsMatrixSummary())
    yield L.gg_pairs_matrix(e.c, ptr(e.sk), ptr(e.lens), N, ptr(rows), 3, F(MIN_ANI), byref(out), byref(n), byref(summary))
    assert out.value is None and n.value == 0 and is_zero(summary)
    pairs, summary = e.ctx.pairs_matrix(e.sk, e.lens, MIN_ANI)
    assert same_pairs(pairs, e.exp) and summary["n_pairs"] == 1 and summary["pair_passes"] == 1


@case("gg_pairs_border_matrix_device", INVALID, "gg_pairs_border_matrix_device: n_old exceeds n")
def _(e):
    d_out, d_count, summary = dev(np.zeros(4, ga.PAIR_DTYPE)), dev(np.zeros(1, np.uint64)), fill(ga._PairsMatrixSummary())
    yield L.gg_pairs_border_matrix_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, N + 1, F(MIN_ANI),
                                          d_out.data_ptr(), 4, d_count.data_ptr(), byref(summary), None)
    assert is_zero(summary) and host(d_count, np.uint64)[0] == 0
    summary = e.ctx.pairs_border_matrix_device(e.d_sk, e.d_lens, N, 1, MIN_ANI, d_out, 4, d_count)
    assert host(d_count, np.uint64)[0] == 1 and same_pairs(host(d_out, ga.PAIR_DTYPE)[:1], e.exp)
    assert summary["n_pairs"] == 1


@case("gg_pairs_border_matrix", INVALID, "gg_pairs_border_matrix: n_old exceeds n")
def _(e):
    out, n, summary = vp(POISON), u64(7), fill(ga._PairsMatrixSummary())
    yield L.gg_pairs_border_matrix(e.c, ptr(e.sk), ptr(e.lens), N, N + 1, F(MIN_ANI), byref(out), byref(n), byref(summary))
    assert out.value is None and n.value == 0 and is_zero(summary)
    pairs, summary = e.ctx.pairs_border_matrix(e.sk, e.lens, 1, MIN_ANI)
    assert same_pairs(pairs, ga.pairs_border_host(e.sk, e.lens, 1, MIN_ANI, k=K)) and summary["n_pairs"] == 1


@case("gg_set_pairs_path", INVALID, "gg_set_pairs_path: unknown path")
def _(e):
    yield L.gg_set_pairs_path(e.c, 3)
    assert e.ctx.pairs_path == "default"
    assert e.ctx.set_pairs_path("auto") == "default" and e.ctx.set_pairs_path("default") == "auto"


@case("gg_pairs_paths_taken", INVALID, "gg_pairs_paths_taken: null argument")
def _(e):
    yield L.gg_pairs_paths_taken(e.c, None)
    assert sorted(e.ctx.pairs_paths_taken()) == sorted(ga.PAIRS_PATHS)


# ---- ani_pairs.hip ------------------------------------------------------------
def named_list():
    p = np.zeros(2, ga.PAIR_DTYPE)
    p["i"], p["j"] = [1, 2], [0, 2]
    return p


@case("gg_ani_pairs", INVALID, "gg_ani_pairs: pair index out of range")
def _(e):
    bad, ani = named_list(), np.full(2, 7, np.float32)
    bad["j"][1] = N
    yield L.gg_ani_pairs(e.c, ptr(e.sk), ptr(e.lens), N, ptr(bad), 2, ptr(ani))
    assert bad["common"].tolist() == [0, 0] and ani.tolist() == [7, 7]
    got, ani = e.ctx.ani_pairs(e.sk, e.lens, named_list())
    exp, exp_ani = ga.ani_pairs_host(e.sk, e.lens, named_list(), k=K)
    assert same_pairs(got, exp) and f32_bits(ani) == f32_bits(exp_ani) and got["common"].tolist() == [S - 2, 20]


@case("gg_ani_pairs_device", INVALID, "gg_ani_pairs_device: null buffer")
def _(e):
    yield L.gg_ani_pairs_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, None, 2, None)
    d_list = dev(named_list())
    e.ctx.ani_pairs_device(e.d_sk, e.d_lens, N, d_list, 2)
    torch_dev().cuda.synchronize()
    assert same_pairs(host(d_list, ga.PAIR_DTYPE), ga.ani_pairs_host(e.sk, e.lens, named_list(), k=K)[0])


CLUSTERS = [[0, 1], [2]]


def validate_call(e, name, first, ani, members=(0, 1, 2), offsets=(0, 2, 3)):
    members, offsets = np.array(members, np.uint32), np.array(offsets, np.uint32)
    summary, bp, ap, n = fill(ga._Validation()), vp(POISON), vp(POISON), u64(7)
    st = getattr(L, name)(e.c, *first, ptr(members), ptr(offsets), len(offsets) - 1, F(ani), *(
        [None] if name == "gg_validate_files" else []), byref(summary), byref(bp), byref(ap), byref(n))
    return st, summary, bp, ap, n


def assert_validation(got, exp):
    assert repr(got) == repr(exp) and same_pairs(got.bad, exp.bad) and f32_bits(got.bad_ani) == f32_bits(exp.bad_ani)


@case("gg_validate_clusters", INVALID, "gg_validate_clusters: ani is NaN")
def _(e):
    st, summary, bp, ap, n = validate_call(e, "gg_validate_clusters", (ptr(e.sk), ptr(e.lens), N), NAN)
    yield st
    assert (bp.value, ap.value, n.value) == (POISON, POISON, 7) and not is_zero(summary)  # kept
    # at 0.9999 the member 1 is too far from its representative 0: one violation
    exp = ga.validate_clusters_host(e.sk, e.lens, CLUSTERS, 0.9999, k=K)
    assert exp.member_bad == 1 and exp.rep_bad == 0
    assert_validation(e.ctx.validate_clusters(e.sk, e.lens, CLUSTERS, 0.9999), exp)


@case("gg_validate_files", INVALID, "gg_validate_files: null argument")
def _(e):
    st, summary, bp, ap, n = validate_call(e, "gg_validate_files", (None, N), MIN_ANI)
    yield st
    assert (bp.value, ap.value, n.value) == (POISON, POISON, 7)  # kept
    exp = ga.validate_clusters_host(e.fsk, e.flens, CLUSTERS, 0.9999, k=K)
    assert_validation(e.ctx.validate_files(e.paths, CLUSTERS, 0.9999), exp)


# ---- ani_matrix.hip -----------------------------------------------------------
def matrix_out(cells):
    return np.full(cells, 7, np.uint32), np.full(cells, 7, np.uint32), np.full(cells, 7, np.float32)


def assert_matrix(got, exp):
    for g, x in zip(got[:2], exp[:2]):
        assert g.tolist() == x.tolist()
    assert f32_bits(got[2]) == f32_bits(exp[2])


@case("gg_ani_matrix", INVALID, "gg_ani_matrix: row index out of range")
def _(e):
    rows, (c, t, a), summary = np.array([0, N], np.uint32), matrix_out(4), fill(ga._MatrixSummary())
    yield L.gg_ani_matrix(e.c, ptr(e.sk), ptr(e.lens), N, ptr(rows), 2, ptr(c), ptr(t), ptr(a), byref(summary))
    assert is_zero(summary) and c.tolist() == [7] * 4
    assert_matrix(e.ctx.ani_matrix(e.sk, e.lens), ga.ani_matrix_host(e.sk, e.lens, k=K))


@case("gg_ani_matrix_device", INVALID, "gg_ani_matrix_device: no output asked for")
def _(e):
    summary = fill(ga._MatrixSummary())
    yield L.gg_ani_matrix_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, None, N, None, None, None,
                                 byref(summary), None)
    assert is_zero(summary)
    d = [dev(x) for x in matrix_out(N * N)]
    e.ctx.ani_matrix_device(e.d_sk, e.d_lens, N, None, N, *d)
    got = (host(d[0], np.uint32), host(d[1], np.uint32), host(d[2], np.float32))
    assert_matrix(got, [x.reshape(-1) for x in ga.ani_matrix_host(e.sk, e.lens, k=K)])


@case("gg_ani_matrix_files", INVALID, "gg_ani_matrix_files: no output asked for")
def _(e):
    summary = fill(ga._MatrixSummary())
    yield L.gg_ani_matrix_files(e.c, paths_arg(e.paths), N, None, None, None, None, byref(summary))
    assert is_zero(summary)
    assert_matrix(e.ctx.ani_matrix_files(e.paths), ga.ani_matrix_host(e.fsk, e.flens, k=K))


GROUP_MEMBERS, GROUP_OFFSETS = np.array([1, 0, 2], np.uint32), np.array([0, 2, 3], np.uint32)


@case("gg_ani_matrix_groups", INVALID, "gg_ani_matrix_groups: row index out of range")
def _(e):
    members, (c, t, a), summary = np.array([1, N, 2], np.uint32), matrix_out(5), fill(ga._MatrixSummary())
    yield L.gg_ani_matrix_groups(e.c, ptr(e.sk), ptr(e.lens), N, ptr(members), ptr(GROUP_OFFSETS), 2, ptr(c), ptr(t),
                                 ptr(a), byref(summary))
    assert is_zero(summary) and c.tolist() == [7] * 5
    got = e.ctx.ani_matrix_groups(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS)
    assert_matrix(got, ga.ani_matrix_groups_host(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS, k=K))


@case("gg_ani_matrix_groups_device", INVALID, "gg_ani_matrix_groups_device: null offsets")
def _(e):
    summary, d_members = fill(ga._MatrixSummary()), dev(GROUP_MEMBERS)
    d = [dev(x) for x in matrix_out(5)]
    yield L.gg_ani_matrix_groups_device(e.c, e.d_sk.data_ptr(), e.d_lens.data_ptr(), N, d_members.data_ptr(), None, 2,
                                        d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), byref(summary), None)
    assert is_zero(summary) and host(d[0], np.uint32).tolist() == [7] * 5
    e.ctx.ani_matrix_groups_device(e.d_sk, e.d_lens, N, d_members, GROUP_OFFSETS, *d)
    got = (host(d[0], np.uint32), host(d[1], np.uint32), host(d[2], np.float32))
    assert_matrix(got, ga.ani_matrix_groups_host(e.sk, e.lens, GROUP_MEMBERS, GROUP_OFFSETS, k=K))


# ---- collection.cpp -----------------------------------------------------------
class Col:
    """A collection of e's three rows, destroyed on exit."""

    def __init__(self, e, rows=N):
        self.e = e
        self.h = e.ctx.collection_create(MIN_ANI)
        if rows:
            e.ctx.collection_add_rows(self.h, e.sk[:rows], e.lens[:rows])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.e.ctx.collection_destroy(self.h)

    def assert_is(self, sk, lens, exp, exp_ani):
        ctx = self.e.ctx
        pairs, ani = ctx.collection_pairs(self.h)
        got_sk, got_lens = ctx.collection_rows(self.h)
        assert same_pairs(pairs, exp) and f32_bits(ani) == f32_bits(exp_ani)
        assert (got_sk == sk).all() and (got_lens == lens).all()
        info = ctx.collection_stat(self.h)[0]
        assert info["n_rows"] == len(lens) and info["n_pairs"] == len(exp)

    def assert_unchanged(self):
        self.assert_is(self.e.sk, self.e.lens, self.e.exp, self.e.exp_ani)


@case("gg_collection_create", INVALID, "gg_collection_create: min_ani is NaN")
def _(e):
    h = vp(POISON)
    yield L.gg_collection_create(e.c, F(NAN), 0, 0, byref(h))
    assert h.value is None
    with Col(e) as col:
        col.assert_unchanged()


def load_call(e, lens, pairs, ani):
    h = vp(POISON)
    st = L.gg_collection_load(e.c, ptr(e.sk), ptr(lens), N, ptr(pairs), ptr(ani), len(pairs), F(MIN_ANI), byref(h))
    return st, h


@case("gg_collection_load", INVALID, "gg_collection_load: the pairs are not strictly ascending by (i, j)")
def _(e):
    pairs = np.zeros(2, ga.PAIR_DTYPE)
    pairs["i"], pairs["j"] = [0, 0], [2, 1]
    st, h = load_call(e, e.lens, pairs, np.array([0.95, 0.95], np.float32))
    yield st
    assert h.value is None
    handle = e.ctx.collection_load(e.sk, e.lens, e.exp, e.exp_ani, MIN_ANI)
    try:
        pairs, ani = e.ctx.collection_pairs(handle)
        assert same_pairs(pairs, e.exp) and f32_bits(ani) == f32_bits(e.exp_ani)
        assert e.ctx.collection_cluster(handle, MIN_ANI).tolist() == exp_rep(e).tolist()
    finally:
        e.ctx.collection_destroy(handle)


@case("gg_collection_load_nan", INVALID, "gg_collection_create: min_ani is NaN")
def _(e):
    h = vp(POISON)
    yield L.gg_collection_load(e.c, ptr(e.sk), ptr(e.lens), N, ptr(e.exp), ptr(e.exp_ani), 1, F(NAN), byref(h))
    assert h.value is None


@case("gg_collection_add_rows", INVALID, "gg_collection_add_rows: sketch longer than sketch_size")
def _(e):
    with Col(e, rows=2) as col:
        added = u64(7)
        yield L.gg_collection_add_rows(col.h, ptr(e.sk[2:]), ptr(np.array([S + 1], np.uint32)), 1, byref(added))
        assert added.value == 0
        col.assert_is(e.sk[:2], e.lens[:2], e.exp, e.exp_ani)
        assert e.ctx.collection_add_rows(col.h, e.sk[2:], e.lens[2:]) == 0
        col.assert_unchanged()


@case("gg_collection_add_rows_device", INVALID, "gg_collection_add_rows_device: null buffer")
def _(e):
    with Col(e, rows=1) as col:
        added = u64(7)
        yield L.gg_collection_add_rows_device(col.h, None, None, 2, byref(added), None)
        assert added.value == 0
        col.assert_is(e.sk[:1], e.lens[:1], e.exp[:0], e.exp_ani[:0])
        d_sk, d_lens = dev(e.sk[1:]), dev(e.lens[1:])
        assert e.ctx.collection_add_rows_device(col.h, d_sk, d_lens, 2) == 1
        col.assert_unchanged()


def assert_add_files(e, col):
    assert e.ctx.collection_add_files(col.h, e.paths) == 1
    col.assert_is(e.fsk, e.flens, e.fexp, e.fexp_ani)


@case("gg_collection_add_files", INVALID, "gg_collection_add_files: null argument")
def _(e):
    with Col(e, rows=0) as col:
        added = u64(7)
        yield L.gg_collection_add_files(col.h, None, 2, None, byref(added))
        assert added.value == 0
        assert_add_files(e, col)


@case("gg_collection_add_files_io", IO, lambda e: e.io_message)
def _(e):
    with Col(e, rows=0) as col:
        added = u64(7)
        yield L.gg_collection_add_files(col.h, paths_arg(e.bad_paths), 4, None, byref(added))
        assert added.value == 0 and e.ctx.collection_stat(col.h)[0]["n_rows"] == 0
        assert_add_files(e, col)


@case("gg_collection_remove", INVALID, "gg_collection_remove: row index out of range")
def _(e):
    with Col(e) as col:
        rows, new_index = np.array([2, N], np.uint32), np.full(N, 7, np.uint32)
        yield L.gg_collection_remove(col.h, ptr(rows), 2, ptr(new_index))
        assert new_index.tolist() == [7] * N
        col.assert_unchanged()
        assert e.ctx.collection_remove(col.h, [2]).tolist() == [0, 1, 0xFFFFFFFF]
        col.assert_is(e.sk[:2], e.lens[:2], e.exp, e.exp_ani)


@case("gg_collection_cluster", INVALID, "gg_collection_cluster: order is not a permutation")
def _(e):
    with Col(e) as col:
        order, rep = np.array([0, 1, 1], np.uint32), np.full(N, 7, np.uint32)
        yield L.gg_collection_cluster(col.h, ptr(order), F(MIN_ANI), ptr(rep))
        assert rep.tolist() == [7] * N
        order = np.array([2, 1, 0], np.uint32)
        exp = ga.cluster_pairs_host(N, ga.relabel_pairs(e.exp, order), e.exp_ani, MIN_ANI)
        assert e.ctx.collection_cluster(col.h, MIN_ANI, order).tolist() == exp.tolist() == [0, 1, 1]
        col.assert_unchanged()


@case("gg_collection_pairs", INVALID, "gg_collection_pairs: null argument")
def _(e):
    with Col(e) as col:
        pp, n = vp(POISON), u64(7)
        yield L.gg_collection_pairs(col.h, byref(pp), None, byref(n))
        assert (pp.value, n.value) == (POISON, 7)  # kept
        col.assert_unchanged()


@case("gg_collection_rows", INVALID, "gg_collection_rows: null argument")
def _(e):
    with Col(e) as col:
        yield L.gg_collection_rows(col.h, None, None)
        col.assert_unchanged()


@pytest.mark.parametrize("fn, status, message", CASES)
def test_failure_then_valid_call(env, fn, status, message):
    g = fn(env)
    st = next(g)
    got = env.error()
    assert st == status
    assert got == (message(env) if callable(message) else message)
    for _ in g:
        raise AssertionError("a case yields once")


# ----------------------------------------------------------------------------
# n_paths == 0 on the three resident files calls: GG_OK, empty results.
# ----------------------------------------------------------------------------
def test_no_paths(env):
    e = env
    pairs, ani, summary = e.ctx.precluster_files_resident([], MIN_ANI)
    assert len(pairs) == 0 and len(ani) == 0
    assert summary == dict(ga._PairsMatrixSummary().as_dict())
    summary = fill(ga._PairsMatrixSummary())
    st, pp, ap, n = files_call(e, "gg_precluster_files_resident", [], MIN_ANI, (byref(summary),))
    assert st == 0 and pp.value and ap.value and n.value == 0 and is_zero(summary)  # (one element each: gg_free both)
    L.gg_free(pp)
    L.gg_free(ap)

    members, offsets, cells, common, total, ani, summary = e.ctx.precluster_matrices_files([], MIN_ANI)
    assert len(members) == 0 and offsets.tolist() == [0] and cells.tolist() == [0]
    assert len(common) == len(total) == len(ani) == 0 and set(summary.values()) == {0}
    st, outs, ng, summary = matrices_call(e, [], MIN_ANI)
    assert st == 0 and all(outs) and ng == 0 and is_zero(summary)
    for o in outs:
        L.gg_free(vp(o))

    st, rep, summary = cluster_resident_call(e, [], MIN_ANI, MIN_ANI)
    assert st == 0 and is_zero(summary) and rep.tolist() == [7]
    assert_cluster_resident(e)
