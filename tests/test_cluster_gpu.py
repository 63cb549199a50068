"""The finch + finch clustering step on the GPU (DESIGN.md 4.5,
galah_amd/csrc/cluster.hip): the inputs of tests/cluster_cases.py through
Context.cluster_pairs must give the rep_of of cluster_pairs_host and of the
reference restatement (tests/cluster_ref.py), bit for bit; then the
device-resident form, the fused file call, the mirrors, a two-member context
and the timing counters."""
import logging
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import galah_amd as ga
from conftest import GOLD_DATA, ROOT

pytestmark = pytest.mark.gpu


def check_device(ctx, case):
    n, pairs, ani, T, exp = case
    got = ctx.cluster_pairs(n, pairs, ani, T)
    assert got.dtype == np.uint32 and len(got) == n
    assert got.tolist() == exp.tolist()
    assert got.tolist() == ga.cluster_pairs_host(n, pairs, ani, T).tolist()


@pytest.mark.parametrize("T", cc.GOLDEN_T)
@pytest.mark.parametrize("min_ani", cc.GOLDEN_MIN_ANI)
def test_golden_pairs(gpu_ctx, min_ani, T):
    check_device(gpu_ctx, cc.golden_case(min_ani, T))


@pytest.mark.parametrize("name", sorted(cc.hand_cases()))
def test_hand_graphs(gpu_ctx, name):
    check_device(gpu_ctx, cc.hand_cases()[name])


def test_pairs_reversed_and_shuffled(gpu_ctx):
    n, pairs, ani, T, exp = cc.golden_case("0.0", "0.98")
    order = np.random.default_rng(5).permutation(len(pairs))
    assert gpu_ctx.cluster_pairs(n, pairs[order][:, ::-1].copy(), ani[order], T).tolist() == exp.tolist()


def test_invalid_arguments(gpu_ctx):
    ok_pairs, ok_ani = [(0, 1), (1, 2)], [0.96, 0.97]
    bad = [
        (3, [(0, 1), (1, 3)], ok_ani, 0.95),
        (3, [(0, 1), (2, 2)], ok_ani, 0.95),
        (3, ok_pairs, [0.96, float("nan")], 0.95),
        (3, ok_pairs, ok_ani, float("nan")),
    ]
    for n, pairs, ani, T in bad:
        with pytest.raises(ga.GalahGpuError) as e:
            gpu_ctx.cluster_pairs(n, pairs, ani, T)
        assert e.value.status == 1
    assert gpu_ctx.cluster_pairs(3, ok_pairs, ok_ani, 0.95).tolist() == [0, 2, 2]


@pytest.mark.parametrize("rising", (False, True))
def test_path_graphs_depth(gpu_ctx, rising):
    """A chain of 20,000 dependent decisions, across 20 workgroup ranges."""
    check_device(gpu_ctx, cc.path_case(rising))
    # launches grow with the ranges the chain crosses (20), never with n
    line = gpu_ctx.info_line()
    rounds = int(line.split("cluster round launches ")[1].split(";")[0].split()[0])
    assert 1 <= rounds <= (cc.PATH_N + 1023) // 1024 + 1


def test_clique_heavy_rows(gpu_ctx):
    """Rows of up to 1,499 strong lower neighbours: scanned by a wave."""
    check_device(gpu_ctx, cc.clique_case())


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs(gpu_ctx, seed):
    check_device(gpu_ctx, cc.random_case(seed))


def test_boundary_graph(gpu_ctx):
    """n just above one workgroup's 1,024 vertices: dependencies cross the range boundary."""
    check_device(gpu_ctx, cc.boundary_case())


def _device_inputs(case, device):
    import torch
    n, pairs, ani, T, exp = case
    p = np.zeros(len(pairs), ga.PAIR_DTYPE)
    p["i"], p["j"] = pairs[:, 0], pairs[:, 1]
    p["common"], p["total"] = 0xDEAD, 0xBEEF  # not read
    d_pairs = torch.from_numpy(p.view(np.uint8).copy()).to(device)
    d_ani = torch.from_numpy(ani.copy()).to(device)
    return d_pairs, d_ani


@pytest.mark.parametrize("which", ("golden", "random", "no_pairs"))
def test_device_form_on_a_stream(gpu_ctx, which):
    import torch
    device = "cuda:%d" % gpu_ctx.device
    case = {"golden": cc.golden_case("0.9", "0.98"), "random": cc.random_case(3),
            "no_pairs": cc.hand_cases()["no_pairs"]}[which]
    n, pairs, ani, T, exp = case
    d_pairs, d_ani = _device_inputs(case, device)
    poison = 0x7FFFFFF0
    d_rep = torch.full((n,), poison, dtype=torch.int32, device=device)
    stream = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu_ctx.cluster_pairs_device(n, d_pairs, d_ani, len(pairs), T, d_rep, stream=stream.cuda_stream)
    stream.synchronize()
    got = d_rep.cpu().numpy().view(np.uint32)
    assert (got != poison).all()  # every entry overwritten
    assert got.tolist() == exp.tolist()


@pytest.mark.parametrize("T", ("0.95", "0.98"))
def test_fused_cluster_files(gpu_ctx, golden, T):
    thr = float(np.float32(0.9))
    exp_pairs, exp_ani = gpu_ctx.precluster_files(golden["paths"], thr)
    rep_of, pairs, ani = gpu_ctx.cluster_files(golden["paths"], thr, float(np.float32(T)))
    assert rep_of.tolist() == cc.golden_rows()[("0.9", T)].tolist()
    assert len(pairs) == 161 and pairs.tobytes() == exp_pairs.tobytes() and ani.tobytes() == exp_ani.tobytes()
    # pairs = ani = n_out = NULL
    alone = gpu_ctx.cluster_files(golden["paths"], thr, float(np.float32(T)), want_pairs=False)
    assert alone.tolist() == rep_of.tolist()


def test_python_mirror_cluster(golden, caplog):
    pre, clu = ga.FinchPreclusterer(0.9), ga.FinchClusterer(0.95)
    assert clu.method_name() == "finch" and clu.get_ani_threshold() == np.float32(0.95)
    with caplog.at_level(logging.INFO, logger="galah"):
        clusters = ga.cluster(golden["paths"], pre, clu)
    assert clusters == ga.clusters_from_reps(cc.golden_rows()[("0.9", "0.95")])
    assert len(clusters) == 5 and sorted(g for c in clusters for g in c) == list(range(27))
    msgs = [r.getMessage() for r in caplog.records]
    # src/clusterer.rs:24-32
    assert msgs[0] == "Preclustering with finch and clustering with finch"
    assert msgs[1] == "Preclustering and clustering methods are the same, so reusing ANI values"


def test_python_mirror_other_clusterer_raises(golden):
    class Skani(ga.FinchClusterer):
        def method_name(self):
            return "skani"

    with pytest.raises(NotImplementedError, match="finch \\+ skani"):
        ga.cluster(golden["paths"][:2], ga.FinchPreclusterer(0.9), Skani(0.95))


def test_finch_clusterer_calculate_ani():
    clu = ga.FinchClusterer(0.95)
    a = clu.calculate_ani(os.path.join(GOLD_DATA, "set1", "1mbp.fna.gz"), os.path.join(GOLD_DATA, "set1", "500kb.fna.gz"))
    assert a == np.float32(0.9808188)  # src/finch.rs:96


def test_two_member_context():
    case = cc.random_case(2)
    n, pairs, ani, T, exp = case
    with ga.Context(k=21, sketch_size=1000, seed=0, devices=[0, 0]) as ctx:
        assert ctx.device_count == 2
        assert ctx.cluster_pairs(n, pairs, ani, T).tolist() == exp.tolist()
        # the step ran on the first member
        ctx.timing_enable(True)
        ctx.cluster_pairs(n, pairs, ani, T)
        assert ctx.member(0).timing_read(ga.KERNEL_CLUSTER)["launches"] > 0
        assert ctx.member(1).timing_read(ga.KERNEL_CLUSTER)["launches"] == 0


def test_timing_counts_pairs(gpu_ctx):
    n, pairs, ani, T, exp = cc.random_case(1)
    gpu_ctx.timing_enable(True)
    try:
        gpu_ctx.cluster_pairs(n, pairs, ani, T)
        t = gpu_ctx.timing_read(ga.KERNEL_CLUSTER)
    finally:
        gpu_ctx.timing_enable(False)
    assert t["launches"] > 0 and t["work"] == len(pairs) and t["ms"] > 0


def test_cpp_mirror_cluster(golden):
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_cluster_mirror")
    lib = os.path.join(ROOT, "galah_amd", "lib")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall",
                           "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cluster_mirror.cpp"),
                           "-L", lib, "-lgalahgpu", "-Wl,-rpath," + lib])
    rep_of = ",".join(str(int(r)) for r in cc.golden_rows()[("0.9", "0.95")])
    r = subprocess.run([exe, GOLD_DATA, rep_of] + golden["names"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
