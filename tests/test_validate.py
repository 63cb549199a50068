"""Named-pair ANI and cluster validation on the host:
gg_ani_pairs_host and gg_validate_clusters_host against the restatement of
tests/validate_ref.py (finch's merge loop, validate_clusters' two loops), the
reader of cluster definition files and the two writers against the
reference's behaviour.  Every comparison is exact: integers against
integers, and every f32 is gg_ani_f32 of those integers.  The device forms
are checked against these in test_validate_gpu.py.  CPU only."""
import io
import os

import numpy as np
import pytest

import galah_amd as ga
import validate_ref as vr
from cluster_cases import golden_rows
from conftest import GOLD


def check_host_pairs(sk, lens, pairs, k=21):
    got, ani = ga.ani_pairs_host(sk, lens, pairs, k=k)
    counts, exp_ani = vr.ani_pairs_ref(sk, lens, pairs, k)
    assert [(int(p["i"]), int(p["j"])) for p in got] == [(int(i), int(j)) for i, j in pairs]
    assert [(int(p["common"]), int(p["total"])) for p in got] == counts
    assert ani.dtype == np.float32 and ani.tobytes() == np.array(exp_ani, dtype=np.float32).tobytes()
    return got, ani


# ---- gg_ani_pairs_host ----------------------------------------------------------
def test_golden_pairs_both_orientations_with_repeats(golden):
    rows = golden["pairs"]
    assert len(rows) == 351
    pairs = ([(i, j) for i, j, _, _, _ in rows] + [(j, i) for i, j, _, _, _ in rows]
             + [(i, j) for i, j, _, _, _ in rows[:40]])
    got, ani = ga.ani_pairs_host(golden["sketches"], golden["lens"], pairs)
    exp = rows + rows + rows[:40]
    assert [(int(p["common"]), int(p["total"])) for p in got] == [(c, t) for _, _, c, t, _ in exp]
    assert ani.tobytes() == np.array([a for _, _, _, _, a in exp], dtype=np.float32).tobytes()
    # and the restatement's merge gives the committed rows too
    assert vr.ani_pairs_ref(golden["sketches"], golden["lens"], pairs[:351])[0] == [(c, t) for _, _, c, t, _ in rows]


@pytest.mark.parametrize("s", (1, 64, 1000, 12000))
def test_edge_lengths(s):
    sk, lens, pairs = vr.edge_case(s)
    got, _ = check_host_pairs(sk, lens, pairs)
    for p in got:
        i, j = int(p["i"]), int(p["j"])
        if lens[i] == 0 or lens[j] == 0:
            assert (p["common"], p["total"]) == (0, 0)
        elif i == j:
            assert (p["common"], p["total"]) == (lens[i], lens[i])


def test_merge_shapes():
    names, sk, lens, pairs = vr.shape_case()
    got, ani = check_host_pairs(sk, lens, pairs)
    at = {(names[int(p["i"])], names[int(p["j"])]): (int(p["common"]), int(p["total"])) for p in got}
    s = int(lens[names.index("a")])
    n_sub = int(lens[names.index("subset")])
    assert at[("a", "a_again")] == (s, s) and at[("a", "a")] == (s, s)
    assert at[("a", "disjoint_above")] == (0, s) == at[("disjoint_above", "a")]  # a ends before the other starts
    # a subset with a smaller last element: it ends first, a is walked up to that element
    last = int(sk[names.index("subset"), n_sub - 1]) // 1000
    assert at[("a", "subset")] == (n_sub, last) == at[("subset", "a")]
    n_sl = int(lens[names.index("subset_same_last")])
    assert at[("a", "subset_same_last")] == (n_sl, s)  # equal last elements: both end together
    assert at[("a", "interleaved")] == (0, 2 * s - 1)
    assert at[("a", "empty")] == (0, 0) == at[("empty", "empty")]
    assert at[("one", "one")] == (1, 1)


def test_other_kmer_length(golden):
    pairs = [(0, 2), (5, 1)]
    _, a21 = check_host_pairs(golden["sketches"], golden["lens"], pairs, k=21)
    _, a31 = check_host_pairs(golden["sketches"], golden["lens"], pairs, k=31)
    assert (a31 > a21).all()


def test_no_pairs(golden):
    got, ani = ga.ani_pairs_host(golden["sketches"], golden["lens"], [])
    assert len(got) == 0 and len(ani) == 0


# ---- reader and writers ----------------------------------------------------------
def _write(tmp_path, text, name="clusters.tsv"):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


def test_reader_well_formed(tmp_path):
    p = _write(tmp_path, "a\ta\na\tb\na\tc\nd\td\ne\te\ne\tf\n")
    assert ga.read_clustering_file(p) == [["a", "b", "c"], ["d"], ["e", "f"]]


def test_reader_member_line_before_any_representative(tmp_path):
    p = _write(tmp_path, "x\ty\nz\tw\na\ta\na\tb\n")
    assert ga.read_clustering_file(p) == [["a", "b"]]
    assert ga.read_clustering_file(_write(tmp_path, "x\ty\n", "only_members.tsv")) == []


def test_reader_does_not_compare_a_member_with_the_open_representative(tmp_path):
    p = _write(tmp_path, "a\ta\nd\tb\nd\td\nd\te\na\tc\n")
    assert ga.read_clustering_file(p) == [["a", "b"], ["d", "e", "c"]]


def test_reader_three_fields_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="exactly 2 fields"):
        ga.read_clustering_file(_write(tmp_path, "a\ta\na\tb\tc\n"))
    with pytest.raises(ValueError, match="exactly 2 fields"):
        ga.read_clustering_file(_write(tmp_path, "a\n", "one_field.tsv"))


def test_reader_empty_file_and_empty_lines(tmp_path):
    assert ga.read_clustering_file(_write(tmp_path, "")) == []
    p = _write(tmp_path, "\na\ta\n\n\na\tb\r\n\nc\tc", "gaps.tsv")
    assert ga.read_clustering_file(p) == [["a", "b"], ["c"]]


def test_reader_does_not_interpret_quotes(tmp_path):
    p = _write(tmp_path, '"a"\t"a"\n"a"\tb"c\n')
    assert ga.read_clustering_file(p) == [['"a"', 'b"c']]


S1D, S2M = "tests/data/abisko4/73.20120800_S1D.21.fna", "tests/data/abisko4/73.20110800_S2M.16.fna"
CMDLINE = {"completeness_4contamination": [S1D, S2M], "parks2020_reduced": [S2M, S1D]}


@pytest.mark.parametrize("name", sorted(CMDLINE))
def test_reference_command_line_outputs(name):
    """The stdout the reference expects of `galah cluster --output-cluster-definition
    /dev/stdout` (tests/test_cmdline.rs:27-29, :53-55): read, and written back."""
    path = os.path.join(GOLD, "cluster_definition_%s.tsv" % name)
    assert ga.read_clustering_file(path) == [CMDLINE[name]]
    genomes = [S1D, S2M]  # the order of --genome-fasta-files
    clusters = [[genomes.index(p) for p in CMDLINE[name]]]
    out = io.BytesIO()
    ga.write_cluster_definition(out, clusters, genomes)
    assert out.getvalue() == open(path, "rb").read()
    text = io.StringIO()
    ga.write_representative_list(text, clusters, genomes)
    assert text.getvalue() == CMDLINE[name][0] + "\n"


def test_writers_golden_clustering(golden, tmp_path):
    names = golden["names"]
    clusters = ga.clusters_from_reps(golden_rows()[("0.9", "0.95")])
    assert [c[0] for c in clusters] == [0, 18, 20, 22, 24]
    exp = "".join("%s\t%s\n" % (names[c[0]], names[g]) for c in clusters for g in c)
    assert exp.count("\n") == 27 and exp.startswith("%s\t%s\n%s\t%s\n" % (names[0], names[0], names[0], names[1]))
    text = io.StringIO()
    ga.write_cluster_definition(text, clusters, names)
    assert text.getvalue() == exp
    path = str(tmp_path / "def.tsv")
    ga.write_cluster_definition(path, clusters, names)
    assert open(path, "rb").read() == exp.encode()
    # read(write(x)) == x
    assert ga.read_clustering_file(path) == [[names[g] for g in c] for c in clusters]
    reps = str(tmp_path / "reps.txt")
    ga.write_representative_list(reps, clusters, names)
    assert open(reps).read() == "".join(names[c[0]] + "\n" for c in clusters)


@pytest.mark.parametrize("clusters", ([], [[0]], [[2], [0], [1]], [[1, 0, 2]]))
def test_write_then_read(tmp_path, clusters):
    genomes = ["g/a.fna", "g/b c.fna", "g/d.fna"]
    path = str(tmp_path / "x.tsv")
    ga.write_cluster_definition(path, clusters, genomes)
    assert ga.read_clustering_file(path) == [[genomes[g] for g in c] for c in clusters]


# ---- gg_validate_clusters_host -----------------------------------------------------
def check_host_validation(sk, lens, clusters, threshold):
    v = ga.validate_clusters_host(sk, lens, clusters, threshold)
    ref = vr.validate_ref(sk, lens, clusters, threshold)
    assert vr.as_tuples(v) == ref
    assert v.ok == (not ref[1] and not ref[3])
    return v


GOLDEN_T = ("0.9", "0.95", "0.97", "0.98", "0.99", "0.995")


@pytest.mark.parametrize("T", GOLDEN_T)
def test_golden_clustering_at_its_own_threshold(golden, T):
    clusters = vr.clusters_of(golden_rows()[("0.0", T)])
    assert clusters == ga.clusters_from_reps(golden_rows()[("0.0", T)])
    v = check_host_validation(golden["sketches"], golden["lens"], clusters, np.float32(T))
    R = len(clusters)
    assert v.ok and len(v.bad) == 0
    assert (v.member_pairs, v.rep_pairs) == (27 - R, R * (R - 1) // 2)


def test_loose_clustering_at_a_tighter_threshold(golden):
    clusters = vr.clusters_of(golden_rows()[("0.9", "0.95")])
    v = check_host_validation(golden["sketches"], golden["lens"], clusters, np.float32(0.98))
    assert (v.member_pairs, v.rep_pairs) == (22, 10)
    assert v.member_bad > 0 and v.rep_bad == 0
    pairs, ani = v.member_violations
    assert (ani < np.float32(0.98)).all() and {int(p["i"]) for p in pairs} <= {0, 18, 20, 22, 24}


def test_tight_clustering_at_a_looser_threshold(golden):
    clusters = vr.clusters_of(golden_rows()[("0.9", "0.98")])
    v = check_host_validation(golden["sketches"], golden["lens"], clusters, np.float32(0.95))
    assert v.rep_bad > 0 and v.member_bad == 0
    pairs, ani = v.rep_violations
    assert (ani >= np.float32(0.95)).all() and (pairs["i"] < pairs["j"]).all()


def test_genome_listed_in_two_clusters(golden):
    # 5 is a member of both clusters and listed twice in the second; the
    # representative 3 is listed again among its own members (skipped)
    clusters = [[0, 5, 1], [3, 5, 3, 5, 20]]
    v = check_host_validation(golden["sketches"], golden["lens"], clusters, np.float32(0.98))
    assert v.member_pairs == 5 and v.rep_pairs == 1
    pairs, _ = v.member_violations
    assert [(int(p["i"]), int(p["j"])) for p in pairs] == sorted((int(p["i"]), int(p["j"])) for p in pairs)
    assert (3, 20) in [(int(p["i"]), int(p["j"])) for p in pairs]


def test_single_cluster_and_all_singletons(golden):
    v = check_host_validation(golden["sketches"], golden["lens"], [list(range(27))], np.float32(0.95))
    assert (v.member_pairs, v.rep_pairs, v.rep_bad) == (26, 0, 0) and v.member_bad > 0
    v = check_host_validation(golden["sketches"], golden["lens"], [[g] for g in range(27)], np.float32(0.95))
    assert (v.member_pairs, v.member_bad, v.rep_pairs) == (0, 0, 351)
    assert v.rep_bad == sum(1 for r in golden["pairs"] if r[4] >= np.float32(0.95))
    v = check_host_validation(golden["sketches"], golden["lens"], [], np.float32(0.95))
    assert v.ok and (v.member_pairs, v.rep_pairs) == (0, 0)


def boundary_pairs(golden):
    """Golden pairs whose f64 ANI lies below its f32 rounding."""
    return [(i, j, c, t, a) for i, j, c, t, a in golden["pairs"] if ga.ani_f64(c, t) < float(a)]


def test_f32_boundary(golden):
    """The rule is on the f32: two singleton representatives whose f64 ANI is
    below the threshold but rounds up to it are a violation; at the next f32
    above they are not."""
    rows = boundary_pairs(golden)
    assert len(rows) == 80
    assert (0, 2, 654, 1265) in [r[:4] for r in rows]
    assert ga.ani_f64(654, 1265) < float(np.float32(0.98174739)) and ga.ani_f32(654, 1265) == np.float32(0.98174739)
    for i, j, c, t, a in rows[:8] + [r for r in rows if r[:2] == (0, 2)]:
        v = check_host_validation(golden["sketches"], golden["lens"], [[i], [j]], a)
        assert (v.rep_pairs, v.rep_bad) == (1, 1)
        assert vr.as_tuples(v)[3] == [(i, j, c, t, a)]
        above = np.nextafter(a, np.float32(2))
        assert above > a
        v = check_host_validation(golden["sketches"], golden["lens"], [[i], [j]], above)
        assert (v.rep_pairs, v.rep_bad) == (1, 0) and v.ok
        # the member rule at the same two thresholds: >= is ok
        assert ga.validate_clusters_host(golden["sketches"], golden["lens"], [[i, j]], a).ok
        assert ga.validate_clusters_host(golden["sketches"], golden["lens"], [[i, j]], above).member_bad == 1


def test_invalid_arguments(golden):
    sk, lens = golden["sketches"], golden["lens"]
    cases = [
        lambda: ga.ani_pairs_host(sk, lens, [(0, 27)]),
        lambda: ga.ani_pairs_host(sk, lens, [(27, 0)]),
        lambda: ga.ani_pairs_host(sk[:, :999], lens, [(0, 1)]),  # lens[g] = 1000 > sketch_size
        lambda: ga.validate_clusters_host(sk, lens, [[0, 1], [2, 27]], 0.95),
        lambda: ga.validate_clusters_host(sk, lens, [[0, 1], [2]], float("nan")),
        lambda: ga.validate_clusters_host(sk, lens, [[0, 1], [], [2]], 0.95),  # an empty cluster
        lambda: ga.validate_clusters_host(sk[:, :999], lens, [[0, 1]], 0.95),
    ]
    for call in cases:
        with pytest.raises(ga.GalahGpuError) as e:
            call()
        assert e.value.status == 1
        assert str(e.value).startswith("gg_") and len(str(e.value)) > 30  # a message naming the entry point


def test_invalid_list_length_and_offsets(golden):
    import ctypes
    L = ga.lib()
    sk = np.ascontiguousarray(golden["sketches"])
    lens = np.ascontiguousarray(golden["lens"])
    one = np.zeros(1, ga.PAIR_DTYPE)
    # m >= 2^31 is refused before the list is read
    st = L.gg_ani_pairs_host(sk.ctypes.data, lens.ctypes.data, 27, 1000, 21, one.ctypes.data, 1 << 31, None)
    assert st == 1 and b"2^31" in L.gg_thread_last_error()
    # offsets that go down
    members = np.array([0, 1, 2, 3], np.uint32)
    offsets = np.array([0, 3, 2, 4], np.uint32)
    out = [ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()]
    summary = ga._Validation()
    st = L.gg_validate_clusters_host(sk.ctypes.data, lens.ctypes.data, 27, 1000, 21, members.ctypes.data,
                                     offsets.ctypes.data, 3, ctypes.c_float(0.95),
                                     ctypes.byref(summary), ctypes.byref(out[0]), ctypes.byref(out[1]),
                                     ctypes.byref(out[2]))
    assert st == 1 and b"offsets" in L.gg_thread_last_error()


def test_abi_version_unchanged():
    assert ga.abi_version() == 7
    assert ga.KERNEL_ANI_PAIRS == 12
