"""The precluster step on the GPU (galah_amd/csrc/precluster.hip):
Context.preclusters over the inputs of tests/preclusters_cases.py must give
what the host forms (partition_preclusters + precluster_pairs, precluster.cpp)
give -- members, offsets and pair_offsets exactly, the local pairs after a
lexsort on (precluster, i, j, src) on both sides, since the host's std::sort
leaves the order of one pair's duplicates open -- and, for the small cases,
what galah's own loops restated in oracle/ give.  Then the device-resident
form, the timing slot, a two-member context and the composition with
cluster_pairs_device."""
import math

import numpy as np
import pytest

import galah_amd as ga
import oracle
import preclusters_cases as pcs
from conftest import load_golden_pairs

pytestmark = pytest.mark.gpu


def _sorted_local(local):
    order = np.lexsort((local["src"], local["j"], local["i"], local["precluster"]))
    return local[order]


def _assert_equal(got, exp):
    members, offsets, local, poff = got
    e_members, e_offsets, e_local, e_poff = exp
    assert members.dtype == np.uint32 and offsets.dtype == np.uint32
    assert members.tolist() == e_members.tolist()
    assert offsets.tolist() == e_offsets.tolist()
    assert poff.dtype == np.uint64 and poff.tolist() == e_poff.tolist()
    assert local.dtype == ga.LOCAL_PAIR_DTYPE and len(local) == len(e_local)
    assert _sorted_local(local).tobytes() == _sorted_local(e_local).tobytes()
    # grouped by precluster, (i, j) ascending inside it, duplicates in ascending src
    key = np.stack([local["precluster"], local["i"], local["j"], local["src"]], axis=1).astype(np.int64)
    if len(key) > 1:
        d = np.diff(key, axis=0)
        first = (d != 0).argmax(axis=1)
        assert (d[np.arange(len(d)), first] >= 0).all()


def _host(n, pairs):
    members, offsets = ga.partition_preclusters(n, pairs)
    local, poff = ga.precluster_pairs(n, pairs, members, offsets)
    return members, offsets, local, poff


def check(ctx, n, pairs, exp=None):
    """ctx.preclusters == partition_preclusters + precluster_pairs."""
    got = ctx.preclusters(n, pairs)
    _assert_equal(got, exp if exp is not None else _host(n, pairs))
    return got


def check_named(ctx, name):
    n, pairs = pcs.all_cases()[name]
    return check(ctx, n, pairs, pcs.host_result(name))


def check_oracle(n, pairs, got):
    """galah's loops (src/clusterer.rs:409-431, :45-57; transform_ids), as tests/test_preclusters.py."""
    members, offsets, local, poff = got
    rows = [(int(a), int(b)) for a, b in zip(pairs["i"], pairs["j"])]
    sets = [members[offsets[s]:offsets[s + 1]].tolist() for s in range(len(offsets) - 1)]
    assert sets == oracle.partition_sketches(n, rows)
    cache = {(min(a, b), max(a, b)): k for k, (a, b) in enumerate(rows)}
    for s, ids in enumerate(sets):
        want = oracle.transform_ids(cache, ids)
        seg = local[int(poff[s]):int(poff[s + 1])]
        assert (seg["precluster"] == s).all()
        assert [(int(r["i"]), int(r["j"])) for r in seg] == sorted(want)
        assert {(int(r["i"]), int(r["j"])): int(r["src"]) for r in seg} == want


def _jump_launches(ctx):
    line = ctx.info_line()
    return int(line.split("precluster jump launches ")[1].split(";")[0].split()[0])


def test_golden_pairs(gpu_ctx):
    n, pairs = pcs.golden_case()
    assert n == 27 and len(pairs) == 161
    check_oracle(n, pairs, check_named(gpu_ctx, "golden"))


def test_clusterer_rs_abisko4_fact(gpu_ctx):
    n, pairs = pcs.abisko4_case()
    members, offsets, _, _ = check_named(gpu_ctx, "abisko4")
    assert [members[offsets[s]:offsets[s + 1]].tolist() for s in range(len(offsets) - 1)] == [[0, 1, 2, 3]]


@pytest.mark.parametrize("name", sorted(pcs.edge_cases()))
def test_edges(gpu_ctx, name):
    n, pairs = pcs.edge_cases()[name]
    got = check_named(gpu_ctx, name)
    check_oracle(n, pairs, got)
    if name == "n0":
        assert len(got[0]) == 0 and got[1].tolist() == [0] and got[3].tolist() == [0]
    if name == "size_tie":
        assert got[0].tolist() == [0, 3, 1, 2] and got[1].tolist() == [0, 2, 4]


def test_index_out_of_range_is_refused(gpu_ctx):
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.preclusters(3, pcs.pair_array([(0, 1), (0, 3)]))
    assert e.value.status == 1
    check(gpu_ctx, 3, pcs.pair_array([(0, 1)]))  # and the context goes on working


def test_partition_only(gpu_ctx):
    n, pairs = pcs.random_case(2)
    members, offsets, local, poff = gpu_ctx.preclusters(n, pairs, with_pairs=False)
    assert local is None and poff is None
    e_members, e_offsets, _, _ = pcs.host_result("random2")
    assert members.tolist() == e_members.tolist() and offsets.tolist() == e_offsets.tolist()


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs(gpu_ctx, seed):
    n, pairs = pcs.random_case(seed)
    assert (pairs["i"] == pairs["j"]).any()
    got = check_named(gpu_ctx, "random%d" % seed)
    if seed < 2:  # (the oracle's loops are quadratic)
        sets = [got[0][got[1][s]:got[1][s + 1]].tolist() for s in range(len(got[1]) - 1)]
        assert sets == oracle.partition_sketches(n, [(int(a), int(b)) for a, b in zip(pairs["i"], pairs["j"])])


@pytest.mark.parametrize("shuffled", (False, True))
def test_path_of_20000(gpu_ctx, shuffled):
    """In order, the hook launch may leave a chain as deep as n: the jump launches stay within their bound."""
    members, offsets, _, _ = check_named(gpu_ctx, "path_shuffled" if shuffled else "path")
    assert offsets.tolist() == [0, pcs.PATH_N]
    assert 1 <= _jump_launches(gpu_ctx) <= math.ceil(math.log2(pcs.PATH_N)) + 1


@pytest.mark.parametrize("hub_last", (False, True))
def test_stars(gpu_ctx, hub_last):
    """Every hook contends on one root; with hub n - 1 the root moves under every compare-and-swap."""
    _, offsets, _, _ = check_named(gpu_ctx, "star_hub_last" if hub_last else "star_hub0")
    assert offsets.tolist() == [0, pcs.STAR_LEAVES + 1]


def test_interleaved_cliques(gpu_ctx):
    n, pairs = pcs.cliques_case()
    assert len(pairs) == 2 * 44850
    members, offsets, local, poff = check_named(gpu_ctx, "cliques")
    # equal sizes: the clique of genome 0 first; positions differ from indices
    assert members[:3].tolist() == [0, 2, 4] and members[300:303].tolist() == [1, 3, 5]
    assert offsets[:3].tolist() == [0, 300, 600] and len(offsets) == 2 + pcs.CLIQUE_SINGLETONS + 1
    assert poff[:3].tolist() == [0, 44850, 89700] and (poff[2:] == 89700).all()


def test_many_equal_sets(gpu_ctx):
    members, offsets, local, poff = check_named(gpu_ctx, "clusters")
    assert len(offsets) == 1001 and (np.diff(offsets.astype(np.int64)) == 10).all()
    firsts = members[offsets[:-1]]
    assert (np.diff(firsts.astype(np.int64)) > 0).all()  # ties by smallest member


@pytest.mark.parametrize("n", (1025, 65537))
def test_key_width(gpu_ctx, n):
    """An index takes 16 bits up to n = 65,536 and 17 from 65,537 on."""
    check_named(gpu_ctx, "n%d" % n)


def _device_run(ctx, n, pairs, stream=None):
    import torch
    device = "cuda:%d" % ctx.device
    m = len(pairs)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).copy()).to(device)
    poison = 0x7FFFFFF0
    d_members = torch.full((max(n, 1),), poison, dtype=torch.int32, device=device)
    d_offsets = torch.full((n + 1,), poison, dtype=torch.int32, device=device)
    d_local = torch.full((max(m, 1) * 4,), poison, dtype=torch.int32, device=device)
    d_poff = torch.full((n + 1,), poison, dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    ns = ctx.preclusters_device(n, d_pairs, m, d_members, d_offsets, d_local, d_poff,
                                stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    members = d_members.cpu().numpy().view(np.uint32)[:n]
    offsets = d_offsets.cpu().numpy().view(np.uint32)[:ns + 1]
    poff = d_poff.cpu().numpy().view(np.uint64)[:ns + 1]
    local = d_local.cpu().numpy().view(ga.LOCAL_PAIR_DTYPE)[:m]
    return members, offsets, local, poff


@pytest.mark.parametrize("name", ("golden", "random3", "n5_no_pairs"))
def test_device_form_on_a_stream(gpu_ctx, name):
    import torch
    n, pairs = pcs.all_cases()[name]
    stream = torch.cuda.Stream(device="cuda:%d" % gpu_ctx.device)
    with torch.cuda.stream(stream):
        got = _device_run(gpu_ctx, n, pairs, stream)
    _assert_equal(got, pcs.host_result(name))
    _assert_equal(got, gpu_ctx.preclusters(n, pairs))


def test_device_form_leaves_out_a_bad_pair(gpu_ctx):
    """One pair with an index >= n: absent, pair_offsets[n_sets] == n_pairs - 1, every other row unchanged."""
    n, pairs = pcs.random_case(3)
    at = len(pairs) // 3
    bad = np.insert(pairs, at, np.array([(5, n, 0, 0)], ga.PAIR_DTYPE))
    members, offsets, local, poff = _device_run(gpu_ctx, n, bad)
    e_members, e_offsets, e_local, e_poff = pcs.host_result("random3")
    assert members.tolist() == e_members.tolist() and offsets.tolist() == e_offsets.tolist()
    assert poff.tolist() == e_poff.tolist() and int(poff[-1]) == len(bad) - 1
    written = local[:len(bad) - 1].copy()
    assert (written["src"] != at).all()
    written["src"] -= (written["src"] > at).astype(np.uint32)  # src counts the injected pair
    assert _sorted_local(written).tobytes() == _sorted_local(e_local).tobytes()
    assert (local[len(bad) - 1:].view(np.uint32) == 0x7FFFFFF0).all()  # the row past them is not written


def test_timing_counts_pairs(gpu_ctx):
    n, pairs = pcs.random_case(1)
    gpu_ctx.timing_enable(True)
    try:
        gpu_ctx.preclusters(n, pairs)
        t = gpu_ctx.timing_read(ga.KERNEL_PRECLUSTER)
    finally:
        gpu_ctx.timing_enable(False)
    assert t["launches"] > 0 and t["work"] == len(pairs) and t["ms"] > 0


def test_two_member_context():
    n, pairs = pcs.random_case(2)
    with ga.Context(k=21, sketch_size=1000, seed=0, devices=[0, 0]) as ctx:
        assert ctx.device_count == 2
        _assert_equal(ctx.preclusters(n, pairs), pcs.host_result("random2"))
        # the step ran on the first member
        ctx.timing_enable(True)
        ctx.preclusters(n, pairs)
        assert ctx.member(0).timing_read(ga.KERNEL_PRECLUSTER)["launches"] > 0
        assert ctx.member(1).timing_read(ga.KERNEL_PRECLUSTER)["launches"] == 0


def test_composition_with_cluster_pairs_device(gpu_ctx):
    """The golden pairs stay on the device for both steps, on one stream:
    every cluster of rep_of lies inside one precluster."""
    import torch
    device = "cuda:%d" % gpu_ctx.device
    n, pairs = pcs.golden_case()
    stored = {(i, j): a for (i, j, c, t, a) in load_golden_pairs()}
    ani = np.array([stored[(int(i), int(j))] for i, j in zip(pairs["i"], pairs["j"])], np.float32)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).copy()).to(device)
    d_ani = torch.from_numpy(ani).to(device)
    d_members = torch.zeros(n, dtype=torch.int32, device=device)
    d_offsets = torch.zeros(n + 1, dtype=torch.int32, device=device)
    d_rep = torch.zeros(n, dtype=torch.int32, device=device)
    stream = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ns = gpu_ctx.preclusters_device(n, d_pairs, len(pairs), d_members, d_offsets, stream=stream.cuda_stream)
        gpu_ctx.cluster_pairs_device(n, d_pairs, d_ani, len(pairs), float(np.float32(0.95)), d_rep,
                                     stream=stream.cuda_stream)
    stream.synchronize()
    members = d_members.cpu().numpy().view(np.uint32)
    offsets = d_offsets.cpu().numpy().view(np.uint32)[:ns + 1]
    rep_of = d_rep.cpu().numpy().view(np.uint32)
    set_of = np.zeros(n, np.int64)
    for s in range(ns):
        set_of[members[offsets[s]:offsets[s + 1]]] = s
    assert (set_of == set_of[rep_of]).all()
    assert rep_of.tolist() == ga.cluster_pairs_host(n, pairs, ani, float(np.float32(0.95))).tolist()
    assert len(set(rep_of.tolist())) >= ns
