"""Clustering from resident sketches on the GPU (DESIGN.md 4.9,
galah_amd/csrc/ani_f32.hip and resident.cpp), through the C ABI with torch
tensors as device memory.

The f32 ANI on the device: over the grid of tests/cpp/test_ani_core.cpp
(total <= 2000, common <= min(total, 1000), total = 0, a few common > total;
1.5M entries) for k = 2, 5, 21, 32 it must equal gg_ani_f32 bit for bit, with
at least one entry and at most 1e-4 of them recomputed by the host; the device
log's own error, |d_ani_f64 - gg_ani_f64|, must stay below E / 8 = 2^-47, so
that the margin E = 2^-44 of ani_core.hpp keeps a factor of 8 over what is
measured here; then the wave and workgroup edges, a margin that flags every
entry (the flagged list overflows and the second pass runs) and a stream.

The resident call: rep_of, the returned pairs and ANI and the summary against
the host composition pairs -> ani_f32 -> cluster_pairs_host ->
partition_preclusters, on the golden sketches, on synthetic rows through both
K2 kernels, past the first pair capacity, and at n = 0, 1, 2; then
cluster_files_resident against cluster_files."""
import ctypes
import functools
import os

import numpy as np
import pytest

import cluster_cases as cc
import galah_amd as ga

pytestmark = pytest.mark.gpu

KS = (2, 5, 21, 32)
E = 2.0 ** -44  # ani_core.hpp kMarginLog2


def torch_dev():
    import torch
    return torch


def to_dev(a):
    """A numpy array's bytes as a device tensor (16-byte records stay 16-byte aligned)."""
    torch = torch_dev()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _hip():
    import torch
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    L = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")  # (the runtime already loaded)
    L.hipMemcpy.restype = ctypes.c_int
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return L


def from_dev(ptr, count, dtype):
    """count records of dtype at a raw device address -> numpy."""
    out = np.zeros(count, dtype)
    if count:
        assert ptr
        assert _hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


# ---------------------------------------------------------------------------
# the f32 ANI
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid():
    t = np.arange(1, 2001, dtype=np.int64)
    per = np.minimum(t, 1000) + 1
    total = np.repeat(t, per)
    common = np.arange(len(total), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    extra = [(0, 0), (1, 0), (7, 0), (1000, 0), (2, 1), (11, 10), (1000, 999), (1000, 1), (4000000000, 3)]
    p = np.zeros(len(total) + len(extra), ga.PAIR_DTYPE)
    p["i"], p["j"] = 0, 1
    p["common"][:len(total)], p["total"][:len(total)] = common, total
    p["common"][len(total):] = [c for c, _ in extra]
    p["total"][len(total):] = [t for _, t in extra]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def grid_ref(k):
    """(gg_ani_f64, its f32) of every grid entry: gg_ani_f32 is (float)gg_ani_f64."""
    p, f = grid(), ga.lib().gg_ani_f64
    v = np.array([f(c, t, k) for c, t in zip(p["common"].tolist(), p["total"].tolist())], np.float64)
    w = v.astype(np.float32)
    for x in range(0, len(p), 1499):  # (and gg_ani_f32 itself on a sample)
        assert ga.ani_f32(int(p["common"][x]), int(p["total"][x]), k).tobytes() == w[x].tobytes()
    v.setflags(write=False)
    w.setflags(write=False)
    return v, w


@functools.lru_cache(maxsize=None)
def grid_device(k):
    torch = torch_dev()
    p = grid()
    d_pairs = to_dev(p)
    d_ani = torch.full((len(p),), float("nan"), dtype=torch.float32, device="cuda")
    d_f64 = torch.full((len(p),), float("nan"), dtype=torch.float64, device="cuda")
    with ga.Context(k=k, sketch_size=1000) as ctx:
        rechecked = ctx.ani_f32_device(d_pairs, len(p), d_ani, d_f64)
    return d_ani.cpu().numpy(), d_f64.cpu().numpy(), rechecked


@pytest.mark.parametrize("k", KS)
def test_ani_bit_equal_over_the_grid(k):
    got, _, rechecked = grid_device(k)
    _, exp = grid_ref(k)
    bad = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
    assert len(bad) == 0, (k, len(bad), grid()[bad[:5]], got[bad[:5]], exp[bad[:5]])
    print("k=%d: %d of %d entries rechecked" % (k, rechecked, len(got)))
    assert 1 <= rechecked <= 1e-4 * len(got)


@pytest.mark.parametrize("k", KS)
def test_device_log_accuracy(k):
    _, got, _ = grid_device(k)
    exp, _ = grid_ref(k)
    worst = float(np.max(np.abs(got - exp)))
    print("k=%d: largest |d_ani_f64 - gg_ani_f64| = %.3g (E/8 = %.3g)" % (k, worst, E / 8))
    assert worst <= E / 8


def inner_entries(count):
    """Indices of `count` grid entries with 0 < common < total, spread over the grid."""
    p = grid()
    idx = np.flatnonzero((p["common"] > 0) & (p["common"] < p["total"]))
    return idx[::len(idx) // count][:count]


def run_ani(ctx, idx, stream=None):
    torch = torch_dev()
    d_pairs = to_dev(grid()[idx])
    d_ani = torch.full((max(len(idx), 1),), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rechecked = ctx.ani_f32_device(d_pairs, len(idx), d_ani, stream=stream)
    torch.cuda.synchronize()
    return d_ani.cpu().numpy()[:len(idx)], rechecked


def test_ani_no_pairs(gpu_ctx):
    assert gpu_ctx.ani_f32_device(0, 0, 0) == 0
    got, rechecked = run_ani(gpu_ctx, np.zeros(0, np.int64))
    assert len(got) == 0 and rechecked == 0


@pytest.mark.parametrize("count", (1, 63, 64, 65, 255, 256, 257))
def test_ani_wave_and_workgroup_edges(gpu_ctx, count):
    # the tail of the grid: its last inner entries, then total = 0 and common > total
    idx = np.arange(len(grid()) - count, len(grid())) if count % 2 else inner_entries(count)
    got, _ = run_ani(gpu_ctx, idx)
    assert got.tobytes() == grid_ref(21)[1][idx].tobytes()


def test_ani_every_entry_flagged_second_pass(gpu_ctx, monkeypatch):
    """E = 2^0: every entry with 0 < common < total is flagged (k = 21: no
    distance above 2), 10,000 of them against a first list of 4,096."""
    idx = inner_entries(10000)
    monkeypatch.setenv("GALAHGPU_TEST_ANI_MARGIN_LOG2", "0")
    got, rechecked = run_ani(gpu_ctx, idx)
    assert rechecked == 10000
    assert got.tobytes() == grid_ref(21)[1][idx].tobytes()
    monkeypatch.delenv("GALAHGPU_TEST_ANI_MARGIN_LOG2")
    got, rechecked = run_ani(gpu_ctx, idx)
    assert rechecked < 100 and got.tobytes() == grid_ref(21)[1][idx].tobytes()


def test_ani_on_a_stream(gpu_ctx):
    torch = torch_dev()
    idx = inner_entries(5000)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got, _ = run_ani(gpu_ctx, idx, stream=stream.cuda_stream)
    assert got.tobytes() == grid_ref(21)[1][idx].tobytes()


# ---------------------------------------------------------------------------
# the resident call
# ---------------------------------------------------------------------------
def ani_f32_of(pairs, k):
    """gg_ani_f32 of every pair (one call per distinct (common, total))."""
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, k) for x in u], np.float32)
    return vals[inv] if len(pairs) else np.zeros(0, np.float32)


def host_composition(ctx, sk, lens, min_ani, T):
    n = len(lens)
    pairs = ctx.pairs(sk, lens, min_ani) if n >= 2 else np.zeros(0, ga.PAIR_DTYPE)
    ani = ani_f32_of(pairs, ctx.k)
    rep_of = ga.cluster_pairs_host(n, pairs, ani, T)
    _, offsets = ga.partition_preclusters(n, pairs) if n else (None, np.zeros(1, np.uint32))
    return pairs, ani, rep_of, len(offsets) - 1, int(offsets[1] - offsets[0]) if n else 0


POISON = 0x7FFFFFF0


def run_resident(ctx, sk, lens, min_ani, T, stream=None):
    """-> (rep_of, summary, pairs sorted by (i, j), their ani)"""
    torch = torch_dev()
    n = len(lens)
    d_sk = to_dev(sk.astype(np.uint64)) if n else 0
    d_lens = to_dev(lens.astype(np.uint32)) if n else 0
    d_rep = torch.full((max(n, 1),), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    summary, p_pairs, p_ani, n_pairs = ctx.cluster_rows_device(d_sk, d_lens, n, min_ani, T, d_rep, stream=stream)
    pairs = from_dev(p_pairs, n_pairs, ga.PAIR_DTYPE)
    ani = from_dev(p_ani, n_pairs, np.float32)
    order = np.lexsort((pairs["j"], pairs["i"]))
    rep_of = d_rep.cpu().numpy().view(np.uint32)[:n]
    assert (rep_of != POISON).all()  # every entry overwritten
    return rep_of, summary, pairs[order], ani[order]


def check_resident(ctx, sk, lens, min_ani, T, passes=1):
    min_ani, T = float(np.float32(min_ani)), float(np.float32(T))
    pairs, ani, rep_of, n_sets, largest = host_composition(ctx, sk, lens, min_ani, T)
    got_rep, summary, got_pairs, got_ani = run_resident(ctx, sk, lens, min_ani, T)
    assert got_pairs.tobytes() == pairs.tobytes()
    assert got_ani.tobytes() == ani.tobytes()
    assert got_rep.tolist() == rep_of.tolist()
    assert summary["n_pairs"] == len(pairs) and summary["ani_rechecked"] <= len(pairs)
    assert (summary["n_preclusters"], summary["largest_precluster"]) == (n_sets, largest)
    assert summary["pair_passes"] == passes
    return got_rep, summary, pairs, ani


GOLDEN_CASES = (("0.9", "0.95"), ("0.9", "0.98"), ("0.95", "0.97"), ("0.9", "0.9"), ("0.95", "0.9"))


@pytest.mark.parametrize("min_ani,T", GOLDEN_CASES)
def test_resident_golden(gpu_ctx, golden, min_ani, T):
    rep_of, summary, pairs, _ = check_resident(gpu_ctx, golden["sketches"], golden["lens"], min_ani, T)
    rows = cc.golden_rows()
    if (min_ani, T) in rows:
        assert rep_of.tolist() == rows[(min_ani, T)].tolist()
    if min_ani == "0.9":
        assert len(pairs) == 161
    # without the summary: the same rep_of
    torch = torch_dev()
    d_rep = torch.full((27,), POISON, dtype=torch.int32, device="cuda")
    none, _, _, n_pairs = gpu_ctx.cluster_rows_device(to_dev(golden["sketches"].astype(np.uint64)),
                                                       to_dev(golden["lens"].astype(np.uint32)), 27,
                                                       float(np.float32(min_ani)), float(np.float32(T)), d_rep,
                                                       want_summary=False)
    assert none is None and n_pairs is None
    assert d_rep.cpu().numpy().view(np.uint32).tolist() == rep_of.tolist()


def test_resident_on_a_stream(gpu_ctx, golden):
    torch = torch_dev()
    stream = torch.cuda.Stream()
    exp = cc.golden_rows()[("0.9", "0.95")]
    with torch.cuda.stream(stream):
        rep_of, summary, _, _ = run_resident(gpu_ctx, golden["sketches"], golden["lens"], float(np.float32(0.9)),
                                             float(np.float32(0.95)), stream=stream.cuda_stream)
    assert rep_of.tolist() == exp.tolist() and summary["n_pairs"] == 161


S_SYNTH = 128


@functools.lru_cache(maxsize=None)
def synth_rows():
    """1,100 rows of 128 hashes in 55 clusters of 20 consecutive rows: a
    member keeps a random share of its cluster's hashes (between all and a
    fifth), the rest its own; clusters share nothing."""
    rng = np.random.default_rng(41)
    n, s = 1100, S_SYNTH
    sk = np.zeros((n, s), np.uint64)
    lens = np.full(n, s, np.uint32)
    for c in range(55):
        base = np.unique(rng.integers(1, 2**60, 2 * s, dtype=np.uint64))[:s]
        for m in range(20):
            keep = base[rng.random(s) < rng.uniform(0.2, 1.0)] if m else base
            own = np.unique(rng.integers(2**60, 2**62, 2 * s, dtype=np.uint64))  # (above every cluster's hashes)
            rng.shuffle(own)
            sk[c * 20 + m] = np.sort(np.concatenate([keep, own[:s - len(keep)]]))
    lens[7] = 0  # an empty row
    sk[7] = 0
    sk.setflags(write=False)
    lens.setflags(write=False)
    return sk, lens


@pytest.fixture(scope="module")
def ctx128():
    with ga.Context(k=21, sketch_size=S_SYNTH) as ctx:
        yield ctx


def paths_delta(ctx, f):
    before = ctx.pair_paths()
    out = f()
    after = ctx.pair_paths()
    return out, {k: after[k] - before[k] for k in after}


def test_resident_index_kernel(ctx128):
    """1,100 rows: above the 512 rows at which K2 takes the inverted index."""
    sk, lens = synth_rows()
    rep_of, summary, pairs, ani = check_resident(ctx128, sk, lens, 0.9, 0.97)
    _, d = paths_delta(ctx128, lambda: run_resident(ctx128, sk, lens, float(np.float32(0.9)), float(np.float32(0.97))))
    assert d["index"] == 1 and d["gate"] == 0, d
    # the shape is what it was made to be: pairs inside clusters only, members and representatives both
    assert len(pairs) >= 5000 and (pairs["i"] // 20 == pairs["j"] // 20).all()
    assert summary["n_preclusters"] >= 55 and 55 < len(set(rep_of.tolist())) < 1100


def test_resident_gate_kernel(ctx128):
    sk, lens = synth_rows()
    _, d = paths_delta(ctx128, lambda: run_resident(ctx128, sk[:100], lens[:100], float(np.float32(0.9)),
                                                    float(np.float32(0.97))))
    assert d["gate"] == 1 and d["index"] == 0, d
    check_resident(ctx128, sk[:100], lens[:100], 0.9, 0.97)


def test_resident_every_pair_passes(ctx128):
    """min_ani = 0: all 4,950 pairs come back, most with ANI exactly 0."""
    sk, lens = synth_rows()
    _, summary, pairs, ani = check_resident(ctx128, sk[:100], lens[:100], 0.0, 0.95)
    assert len(pairs) == 4950 and (ani == 0).sum() > len(ani) // 2 and (ani > 0.95).any()
    assert summary["n_preclusters"] == 1 and summary["largest_precluster"] == 100


def test_resident_capacity_retry():
    """1,500 rows of 16 hashes that all share 12 of them: every one of the
    1,124,250 pairs passes, more than the first capacity of 2^20."""
    rng = np.random.default_rng(43)
    n, s = 1500, 16
    shared = np.arange(1, 13, dtype=np.uint64) * np.uint64(1 << 40)
    pool = np.arange(1, 9, dtype=np.uint64) * np.uint64(1 << 56)  # (above the shared ones)
    sk = np.zeros((n, s), np.uint64)
    for i in range(n):
        sk[i] = np.concatenate([shared, np.sort(rng.choice(pool, 4, replace=False))])
    lens = np.full(n, s, np.uint32)
    with ga.Context(k=21, sketch_size=s) as ctx:
        _, summary, pairs, ani = check_resident(ctx, sk, lens, 0.9, 0.995, passes=2)
    assert summary["n_pairs"] == n * (n - 1) // 2 > 1 << 20
    assert len(np.unique(ani)) >= 3


@pytest.mark.parametrize("n", (0, 1, 2))
def test_resident_tiny(gpu_ctx, golden, n):
    sk, lens = golden["sketches"][[0, 0]][:n], golden["lens"][[0, 0]][:n]
    rep_of, summary, pairs, ani = check_resident(gpu_ctx, sk, lens, 0.9, 0.95, passes=1 if n == 2 else 0)
    assert rep_of.tolist() == [0] * n
    assert summary["n_pairs"] == (1 if n == 2 else 0) and summary["n_preclusters"] == min(n, 1)
    if n == 2:
        assert ani.tolist() == [1.0]


def test_resident_invalid_arguments(gpu_ctx, golden):
    torch = torch_dev()
    d_sk, d_lens = to_dev(golden["sketches"].astype(np.uint64)), to_dev(golden["lens"].astype(np.uint32))
    d_rep = torch.zeros(27, dtype=torch.int32, device="cuda")
    for min_ani, T in ((float("nan"), 0.95), (0.9, float("nan"))):
        with pytest.raises(ga.GalahGpuError) as e:
            gpu_ctx.cluster_rows_device(d_sk, d_lens, 27, min_ani, T, d_rep)
        assert e.value.status == 1
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.cluster_rows_device(d_sk, d_lens, 27, 0.9, 0.95, 0)
    assert e.value.status == 1
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.cluster_files_resident(golden["paths"], float("nan"), 0.95)
    assert e.value.status == 1


# ---------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", ("0.95", "0.98"))
def test_cluster_files_resident(gpu_ctx, golden, T):
    thr, t = float(np.float32(0.9)), float(np.float32(T))
    exp = gpu_ctx.cluster_files(golden["paths"], thr, t, want_pairs=False)
    pairs, _ = gpu_ctx.precluster_files(golden["paths"], thr)
    _, offsets = ga.partition_preclusters(27, pairs)
    rep_of, summary = gpu_ctx.cluster_files_resident(golden["paths"], thr, t)
    assert rep_of.tolist() == exp.tolist() == cc.golden_rows()[("0.9", T)].tolist()
    assert summary["n_pairs"] == len(pairs) == 161 and summary["pair_passes"] == 1
    assert summary["n_preclusters"] == len(offsets) - 1
    assert summary["largest_precluster"] == int(offsets[1] - offsets[0])
    # a two-member context takes cluster_files' path: the same rep_of, the
    # same partition (ani_rechecked and pair_passes are the device form's: 0)
    with ga.Context(k=21, sketch_size=1000, seed=0, devices=[0, 0]) as two:
        assert two.device_count == 2
        rep2, sum2 = two.cluster_files_resident(golden["paths"], thr, t)
    assert rep2.tolist() == rep_of.tolist()
    for f in ("n_pairs", "n_preclusters", "largest_precluster"):
        assert sum2[f] == summary[f], f
    assert sum2["ani_rechecked"] == 0 and sum2["pair_passes"] == 0


def test_cluster_files_resident_tiny(gpu_ctx, golden):
    rep_of, summary = gpu_ctx.cluster_files_resident([], 0.9, 0.95)
    assert len(rep_of) == 0 and summary["n_preclusters"] == 0
    rep_of, summary = gpu_ctx.cluster_files_resident(golden["paths"][:1], 0.9, 0.95)
    assert rep_of.tolist() == [0] and summary["n_preclusters"] == 1 and summary["largest_precluster"] == 1
