"""Named-pair ANI and cluster validation on the GPU (DESIGN.md 4.6,
galah_amd/csrc/ani_pairs.hip): Context.ani_pairs must give, bit for bit, what
ani_pairs_host gives (itself checked against the merge restatement in
test_validate.py) on both paths of the kernel -- rows staged in LDS and rows
searched in global memory -- and Context.validate_clusters what
validate_clusters_host gives on every case of test_validate.py, the f32
boundary included; then the device-resident form, the flow from files, the
mirrors and the timing counter."""
import functools
import logging
import os
import subprocess

import numpy as np
import pytest

import galah_amd as ga
import validate_ref as vr
from cluster_cases import golden_rows
from conftest import GOLD_DATA, ROOT

pytestmark = pytest.mark.gpu


def check_pairs(ctx, sk, lens, pairs):
    exp, exp_ani = ga.ani_pairs_host(sk, lens, pairs, k=ctx.k)
    got, ani = ctx.ani_pairs(sk, lens, pairs)
    assert got.dtype == ga.PAIR_DTYPE and len(got) == len(exp)
    assert got.tobytes() == exp.tobytes()
    assert ani.dtype == np.float32 and ani.tobytes() == exp_ani.tobytes()
    return got


# ---- gg_ani_pairs ---------------------------------------------------------------
def test_golden_pairs_shuffled_with_repeats(gpu_ctx, golden):
    rows = golden["pairs"]
    pairs = np.array([(i, j) for i, j, _, _, _ in rows] + [(j, i) for i, j, _, _, _ in rows[::3]]
                     + [(i, j) for i, j, _, _, _ in rows[:50]], dtype=np.uint32)
    order = np.random.default_rng(11).permutation(len(pairs))
    got = check_pairs(gpu_ctx, golden["sketches"], golden["lens"], pairs[order])
    table = {(i, j): (c, t) for i, j, c, t, _ in rows}
    for p in got:
        i, j = int(p["i"]), int(p["j"])
        assert (int(p["common"]), int(p["total"])) == table[(min(i, j), max(i, j))]


@pytest.mark.parametrize("lds", ("1", "0"))
@pytest.mark.parametrize("s", (64, 1000))
def test_edge_lengths_staged_rows(s, lds, monkeypatch):
    """Every row fits the wave's LDS slice: lengths either side of 64 (one
    round of the wave), empty rows, i == j.  With GALAHGPU_ANI_PAIRS_LDS=0 the
    same rows are searched in global memory."""
    sk, lens, pairs = vr.edge_case(s)
    monkeypatch.setenv("GALAHGPU_ANI_PAIRS_LDS", lds)
    with ga.Context(k=21, sketch_size=s) as ctx:
        check_pairs(ctx, sk, lens, pairs)


@pytest.mark.parametrize("s,lens", ((4096, (2047, 2048, 2049, 4096)), (12000, (1, 2049, 11999, 12000))))
def test_long_rows_searched_in_global_memory(s, lens):
    """4 genomes; a staged row of up to 2,048 hashes takes the LDS path, a
    longer one is searched in global memory: lengths either side of the slice."""
    sk, ln = vr.synth_rows(s, list(lens), 7 + s)
    pairs = [(i, j) for i in range(4) for j in range(4)]
    with ga.Context(k=21, sketch_size=s) as ctx:
        check_pairs(ctx, sk, ln, pairs)


def test_merge_shapes(gpu_ctx):
    names, sk, lens, pairs = vr.shape_case(1000)
    check_pairs(gpu_ctx, sk, lens, pairs)


def test_list_longer_than_one_grid_pass(gpu_ctx, golden):
    """70,000 entries: more pairs than the launch has waves, so every wave's
    grid-stride loop wraps."""
    rng = np.random.default_rng(3)
    pairs = rng.integers(0, 27, size=(70000, 2), dtype=np.uint32)
    got = check_pairs(gpu_ctx, golden["sketches"], golden["lens"], pairs)
    same = pairs[:, 0] == pairs[:, 1]
    assert same.any() and (got["common"][same] == 1000).all() and (got["total"][same] == 1000).all()


@functools.lru_cache(maxsize=None)
def many_small_rows():
    n, s = 5001, 64
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(1, 1 << 62, size=400, dtype=np.uint64))[:256]
    sk = np.sort(np.stack([rng.choice(pool, size=s, replace=False) for _ in range(n)]), axis=1)
    return sk, np.full(n, s, dtype=np.uint32)


def test_one_genome_with_many_partners_then_many_with_one():
    sk, lens = many_small_rows()
    n = len(lens)
    heavy = [(0, j) for j in range(1, 5001)]
    light = [(i, (i * 7 + 3) % n) for i in range(1, 5001)]
    with ga.Context(k=21, sketch_size=64) as ctx:
        got = check_pairs(ctx, sk, lens, heavy + light)
    assert got["common"].max() > 0 and (got["total"] >= got["common"]).all()


def test_empty_and_single_lists(gpu_ctx, golden):
    got, ani = gpu_ctx.ani_pairs(golden["sketches"], golden["lens"], [])
    assert len(got) == 0 and len(ani) == 0
    got = check_pairs(gpu_ctx, golden["sketches"], golden["lens"], [(2, 0)])
    assert (int(got[0]["common"]), int(got[0]["total"])) == (654, 1265)


def test_invalid_arguments(gpu_ctx, golden):
    sk, lens = golden["sketches"], golden["lens"]
    calls = [
        lambda: gpu_ctx.ani_pairs(sk, lens, [(0, 1), (27, 1)]),
        lambda: gpu_ctx.validate_clusters(sk, lens, [[0, 1], [27]], 0.95),
        lambda: gpu_ctx.validate_clusters(sk, lens, [[0, 1], [2]], float("nan")),
        lambda: gpu_ctx.validate_clusters(sk, lens, [[0, 1], [], [2]], 0.95),
    ]
    for call in calls:
        with pytest.raises(ga.GalahGpuError) as e:
            call()
        assert e.value.status == 1 and str(e.value).startswith("gg_")
    too_long = lens.copy()
    too_long[3] = 1001
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.ani_pairs(sk, too_long, [(0, 1)])
    assert e.value.status == 1


# ---- gg_ani_pairs_device --------------------------------------------------------
def test_device_form_on_a_stream(gpu_ctx, golden):
    import torch
    device = "cuda:%d" % gpu_ctx.device
    rng = np.random.default_rng(17)
    ij = rng.integers(0, 27, size=(3000, 2), dtype=np.uint32)
    lst = np.zeros(len(ij), ga.PAIR_DTYPE)
    lst["i"], lst["j"] = ij[:, 0], ij[:, 1]
    out_of_range = {100: (27, 0), 101: (3, 27), 2999: (0xFFFFFFFF, 0xFFFFFFFF), 0: (5, 1 << 31)}
    for at, (i, j) in out_of_range.items():
        lst[at]["i"], lst[at]["j"] = i, j
    lst["common"], lst["total"] = 0xDEAD, 0xBEEF  # overwritten, every entry
    inside = np.array([at not in out_of_range for at in range(len(lst))])
    exp, _ = ga.ani_pairs_host(golden["sketches"], golden["lens"], lst[inside])

    d_sk = torch.from_numpy(golden["sketches"].view(np.int64).copy()).to(device)
    d_len = torch.from_numpy(golden["lens"].view(np.int32).copy()).to(device)
    d_list = torch.from_numpy(lst.view(np.uint8).copy()).to(device)
    stream = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu_ctx.ani_pairs_device(d_sk, d_len, 27, d_list, len(lst), stream=stream.cuda_stream)
    stream.synchronize()
    got = d_list.cpu().numpy().view(ga.PAIR_DTYPE)
    assert got["i"].tolist() == lst["i"].tolist() and got["j"].tolist() == lst["j"].tolist()
    assert got[inside].tobytes() == exp.tobytes()
    for at in out_of_range:
        assert (int(got[at]["common"]), int(got[at]["total"])) == (0, 0)


# ---- gg_validate_clusters ---------------------------------------------------------
def check_validation(ctx, sk, lens, clusters, threshold):
    exp = ga.validate_clusters_host(sk, lens, clusters, threshold, k=ctx.k)
    got = ctx.validate_clusters(sk, lens, clusters, threshold)
    assert (got.member_pairs, got.member_bad, got.rep_pairs, got.rep_bad) == \
        (exp.member_pairs, exp.member_bad, exp.rep_pairs, exp.rep_bad)
    assert got.bad.tobytes() == exp.bad.tobytes() and got.bad_ani.tobytes() == exp.bad_ani.tobytes()
    assert got.ok == exp.ok
    return got


@pytest.mark.parametrize("T", ("0.9", "0.95", "0.97", "0.98", "0.99", "0.995"))
def test_golden_clustering_at_its_own_threshold(gpu_ctx, golden, T):
    clusters = ga.clusters_from_reps(golden_rows()[("0.0", T)])
    v = check_validation(gpu_ctx, golden["sketches"], golden["lens"], clusters, np.float32(T))
    assert v.ok and v.member_pairs == 27 - len(clusters)


def test_clusterings_at_other_thresholds(gpu_ctx, golden):
    sk, lens = golden["sketches"], golden["lens"]
    loose = ga.clusters_from_reps(golden_rows()[("0.9", "0.95")])
    v = check_validation(gpu_ctx, sk, lens, loose, np.float32(0.98))
    assert v.member_bad > 0 and v.rep_bad == 0 and (v.member_pairs, v.rep_pairs) == (22, 10)
    tight = ga.clusters_from_reps(golden_rows()[("0.9", "0.98")])
    v = check_validation(gpu_ctx, sk, lens, tight, np.float32(0.95))
    assert v.rep_bad > 0 and v.member_bad == 0


def test_repeated_genomes_single_cluster_singletons(gpu_ctx, golden):
    sk, lens = golden["sketches"], golden["lens"]
    v = check_validation(gpu_ctx, sk, lens, [[0, 5, 1], [3, 5, 3, 5, 20]], np.float32(0.98))
    assert v.member_pairs == 5 and v.rep_pairs == 1
    v = check_validation(gpu_ctx, sk, lens, [list(range(27))], np.float32(0.95))
    assert (v.member_pairs, v.rep_pairs) == (26, 0)
    v = check_validation(gpu_ctx, sk, lens, [[g] for g in range(27)], np.float32(0.95))
    assert (v.member_pairs, v.rep_pairs) == (0, 351) and v.rep_bad > 0
    # a threshold of 0: every pair of representatives is a violation, none of the members
    v = check_validation(gpu_ctx, sk, lens, [[g] for g in range(27)], np.float32(0.0))
    assert v.rep_bad == 351
    v = check_validation(gpu_ctx, sk, lens, [], np.float32(0.95))
    assert v.ok


def test_f32_boundary_on_the_device_pair_path(gpu_ctx, golden):
    """Two singleton representatives whose f64 ANI is below the threshold and
    rounds up to it: the all-pairs path at the threshold itself would drop
    them (its test is on the f64); at the lowered threshold they are found
    and reported, and at the next f32 above they are not."""
    sk, lens = golden["sketches"], golden["lens"]
    rows = [r for r in golden["pairs"] if ga.ani_f64(r[2], r[3]) < float(r[4])]
    assert len(rows) == 80
    for i, j, c, t, a in rows[:6] + [r for r in rows if r[:2] == (0, 2)]:
        two = np.stack([sk[i], sk[j]])
        assert len(gpu_ctx.pairs(two, lens[[i, j]], float(a))) == 0  # (what the superset threshold is for)
        v = check_validation(gpu_ctx, sk, lens, [[i], [j]], a)
        assert v.rep_bad == 1 and vr.as_tuples(v)[3] == [(i, j, c, t, a)]
        v = check_validation(gpu_ctx, sk, lens, [[i], [j]], np.nextafter(a, np.float32(2)))
        assert v.rep_bad == 0 and v.ok


@functools.lru_cache(maxsize=None)
def many_reps_case():
    """360 genomes of 60 families: five representatives and one member each.
    A family's rows are draws of 1,000 hashes from the family's pool, whose
    size (1,100 .. 4,000) sets how much two of them share: ANI from ~0.995
    down to ~0.93 inside a family, 0 between families."""
    rng = np.random.default_rng(77)
    s, fam = 1000, 60
    rows, clusters = [], []
    for f in range(fam):
        pool = np.unique(rng.integers(1, 1 << 63, size=4200, dtype=np.uint64))[:1100 + (2900 * f) // (fam - 1)]
        first = len(rows)
        for _ in range(6):
            rows.append(np.sort(rng.choice(pool, size=s, replace=False)))
        clusters += [[first, first + 5]] + [[first + r] for r in range(1, 5)]
    return np.stack(rows), np.full(len(rows), s, dtype=np.uint32), clusters


@pytest.mark.parametrize("kernel", ("auto", "index"))
def test_three_hundred_representatives(kernel):
    """The representative side over 300 rows: several 64-genome tiles; with
    the inverted index forced, through the index path."""
    sk, lens, clusters = many_reps_case()
    assert len(clusters) == 300
    old = os.environ.get("GALAHGPU_PAIRS_KERNEL")
    if kernel == "index":
        os.environ["GALAHGPU_PAIRS_KERNEL"] = "index"
    try:
        with ga.Context(k=21, sketch_size=1000) as ctx:
            v = check_validation(ctx, sk, lens, clusters, np.float32(0.95))
            assert (v.member_pairs, v.rep_pairs) == (60, 300 * 299 // 2)
            assert 0 < v.rep_bad < 600 and 0 < v.member_bad < 60
            # a threshold that is one of the pairs' own f32
            _, ani = ga.ani_pairs_host(sk, lens, [(clusters[1][0], clusters[2][0])])
            v = check_validation(ctx, sk, lens, clusters, ani[0])
            assert (clusters[1][0], clusters[2][0]) in [(int(p["i"]), int(p["j"])) for p in v.rep_violations[0]]
            paths = ctx.pair_paths()
            assert (paths["index"] == 2) if kernel == "index" else (paths["gate"] == 2)
    finally:
        if kernel == "index":
            if old is None:
                del os.environ["GALAHGPU_PAIRS_KERNEL"]
            else:
                os.environ["GALAHGPU_PAIRS_KERNEL"] = old


def test_two_member_context(golden):
    sk, lens = golden["sketches"], golden["lens"]
    clusters = ga.clusters_from_reps(golden_rows()[("0.9", "0.98")])
    with ga.Context(k=21, sketch_size=1000, seed=0, devices=[0, 0]) as ctx:
        check_validation(ctx, sk, lens, clusters, np.float32(0.95))
        ctx.timing_enable(True)
        check_pairs(ctx, sk, lens, [(0, 1), (2, 3)])
        assert ctx.member(0).timing_read(ga.KERNEL_ANI_PAIRS)["launches"] == 1
        assert ctx.member(1).timing_read(ga.KERNEL_ANI_PAIRS)["launches"] == 0


def test_timing_counts_listed_pairs(gpu_ctx, golden):
    pairs = [(i, j) for i in range(27) for j in range(27)]
    gpu_ctx.timing_enable(True)
    try:
        gpu_ctx.ani_pairs(golden["sketches"], golden["lens"], pairs)
        t = gpu_ctx.timing_read(ga.KERNEL_ANI_PAIRS)
    finally:
        gpu_ctx.timing_enable(False)
    assert t["launches"] == 1 and t["work"] == len(pairs) and t["ms"] > 0


# ---- from files ------------------------------------------------------------------------
def test_validate_clusters_from_a_definition_file(golden, tmp_path, caplog):
    paths = golden["paths"]
    clusters = ga.cluster(paths, ga.FinchPreclusterer(0.9), ga.FinchClusterer(0.95))
    definition = str(tmp_path / "clusters.tsv")
    ga.write_cluster_definition(definition, clusters, paths)
    assert ga.read_clustering_file(definition) == [[paths[g] for g in c] for c in clusters]

    with caplog.at_level(logging.INFO, logger="galah"):
        v = ga.validate_clusters(definition, 0.95)
    assert v.ok and (v.member_pairs, v.rep_pairs) == (22, 10)
    assert v.member_violation_paths == [] and v.rep_violation_paths == []
    msgs = [r.getMessage() for r in caplog.records]
    assert "Read in 5 clusters" in msgs and not [r for r in caplog.records if r.levelno >= logging.ERROR]

    # the file's genomes in order of appearance, for the restatement
    order = [g for c in clusters for g in c]
    assert v.genomes == [paths[g] for g in order]
    pos = {g: x for x, g in enumerate(order)}
    sk, lens = golden["sketches"][order], golden["lens"][order]
    ref = vr.validate_ref(sk, lens, [[pos[g] for g in c] for c in clusters], np.float32(0.98))
    caplog.clear()
    with caplog.at_level(logging.ERROR, logger="galah"):
        v = ga.validate_clusters(definition, 0.98)
    assert not v.ok and vr.as_tuples(v) == ref
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert errors == vr.error_lines(ref, v.genomes) and len(errors) == v.member_bad > 0
    assert errors[0].startswith("finch ANI between %s and " % paths[clusters[0][0]])

    # debug level: the "ok" lines too, one line per compared pair in all
    caplog.clear()
    with caplog.at_level(logging.DEBUG, logger="galah"):
        ga.validate_clusters(definition, 0.98)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("finch ANI between ")]
    assert len(lines) == 22 + 10 and sum(" is ok: " in x for x in lines) == 32 - len(errors)

    # the sketch cache: a second call reads no genome file
    cache = str(tmp_path / "sketches")
    first = ga.validate_clusters(definition, 0.95, sketch_cache_dir=cache)
    second = ga.validate_clusters(definition, 0.95, sketch_cache_dir=cache)
    assert first.n_cached == 0 and second.n_cached == 27 and second.ok
    assert vr.as_tuples(second) == vr.as_tuples(first)


def test_validate_files_entry_point(gpu_ctx, golden):
    clusters = ga.clusters_from_reps(golden_rows()[("0.9", "0.95")])
    exp = ga.validate_clusters_host(golden["sketches"], golden["lens"], clusters, np.float32(0.98))
    got = gpu_ctx.validate_files(golden["paths"], clusters, np.float32(0.98))
    assert vr.as_tuples(got) == vr.as_tuples(exp)


def test_calculate_ani_many(golden):
    clu = ga.FinchClusterer(0.95)
    p = golden["paths"]
    named = [(p[0], p[2]), (p[20], p[21]), (p[2], p[0]),
             (os.path.join(GOLD_DATA, "set1", "1mbp.fna.gz"), os.path.join(GOLD_DATA, "set1", "500kb.fna.gz"))]
    many = clu.calculate_ani_many(named)
    assert [type(a) for a in many] == [np.float32] * 4
    assert many == [clu.calculate_ani(a, b) for a, b in named]
    assert many[0] == many[2] == np.float32(0.98174739) and many[3] == np.float32(0.9808188)  # src/finch.rs:96
    assert clu.calculate_ani_many([]) == []


def test_cpp_mirror_validate(golden, tmp_path):
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_validate_mirror")
    lib = os.path.join(ROOT, "galah_amd", "lib")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall",
                           "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_validate_mirror.cpp"),
                           "-L", lib, "-lgalahgpu", "-Wl,-rpath," + lib])
    r = subprocess.run([exe, GOLD_DATA, str(tmp_path)] + golden["names"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert out[0] == "ok"
    # the error lines at 0.98 are the restatement's
    clusters = ga.clusters_from_reps(golden_rows()[("0.9", "0.95")])
    order = [g for c in clusters for g in c]
    pos = {g: x for x, g in enumerate(order)}
    ref = vr.validate_ref(golden["sketches"][order], golden["lens"][order], [[pos[g] for g in c] for c in clusters],
                          np.float32(0.98))
    genomes = [os.path.join(GOLD_DATA, golden["names"][g] + ".gz") for g in order]
    assert [x[2:] for x in out[1:]] == vr.error_lines(ref, genomes)
