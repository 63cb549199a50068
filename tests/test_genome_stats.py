"""Genome assembly statistics on the host (gg_genome_stats_files and its
Python mirror): parity with galah's calculate_genome_stats (reference
src/genome_stats.rs:11-51).  CPU only.

The reference is `restate` below: a plain-Python restatement of that
function over the records as the packer walks them.  The reference pins it
with two exact answers (src/genome_stats.rs:61-87), asserted here as literals
against both the restatement and the library; every other case compares the
library with the restatement.  The needletail source is not at hand, so what
a record's sequence holds ("Genome assembly statistics") rests on
those two answers alone.
"""
import gzip
import os

import pytest

import galah_amd as ga
from conftest import GOLD, golden_path


def records(data):
    """The sequence bytes of every record, as pack.cpp's record walk cuts
    them: FASTA records run to the next line that starts with '>'; a FASTQ
    record is the line after its '@' line, then two lines are skipped."""
    i, n = 0, len(data)

    def line_end(at):  # the index after the line that holds `at`
        nl = data.find(b"\n", at)
        return n if nl < 0 else nl + 1

    while i < n:
        tag = data[i:i + 1]
        i = line_end(i)
        start = i
        if tag == b">":
            while i < n and data[i:i + 1] != b">":
                i = line_end(i)
            yield data[start:i]
        else:
            i = line_end(i)
            yield data[start:i]
            for _ in range(2):
                if i < n:
                    i = line_end(i)


def restate(data):
    """src/genome_stats.rs:11-51 -> (num_contigs, num_ambiguous_bases, n50, total_bases)."""
    lens, amb = [], 0
    for seq in records(data):
        lens.append(len(seq) - seq.count(b"\n") - seq.count(b"\r"))  # num_bases
        amb += seq.count(b"N") + seq.count(b"n")
    total = sum(lens)
    cutoff, run, n50 = total // 2, 0, None
    for length in sorted(lens):
        run += length
        if run >= cutoff:
            n50 = length
            break
    return len(lens), amb, n50, total


def as_tuple(s):
    return s.num_contigs, s.num_ambiguous_bases, s.n50, s.total_bases


def load_fixture():
    rows = {}
    with open(os.path.join(GOLD, "genome_stats.tsv")) as f:
        next(f)
        for line in f:
            name, c, a, n50, total = line.split("\t")
            rows[name] = (int(c), int(a), int(n50), int(total))
    return rows


REF_ROWS = {"abisko4/73.20110600_S2D.10.fna": (161, 6506, 8289),  # src/genome_stats.rs:61-73
            "set1/1mbp.fna": (1, 0, 1000000)}                      # src/genome_stats.rs:75-87


def test_restatement_gives_the_reference_answers():
    for name, want in REF_ROWS.items():
        with gzip.open(golden_path(name), "rb") as f:
            assert restate(f.read())[:3] == want, name


def test_golden_genomes_equal_the_fixture(golden):
    fixture = load_fixture()
    assert sorted(fixture) == sorted(golden["names"]) and len(fixture) == 27
    got = ga.genome_stats(golden["paths"])
    for name, s in zip(golden["names"], got):
        assert as_tuple(s) == fixture[name], name
    for name, want in REF_ROWS.items():
        s = got[golden["names"].index(name)]
        assert (s.num_contigs, s.num_ambiguous_bases, s.n50) == want
        assert s == ga.GenomeAssemblyStats(*want)
    assert fixture["abisko4/73.20110600_S2D.10.fna"] == (161, 6506, 8289, 1149523)
    assert fixture["set1/1mbp.fna"] == (1, 0, 1000000, 1000000)


SEQ = b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCCATGCAAGTC"
EDGES = {
    "crlf": b">x desc\r\nACGTN\r\nNNAC\r\n>y\r\nGG\r\n",
    "no_trailing_newline": b">x\nACGT\nACN",
    "empty_records": b">a\n>b\n>c\nACGT\n>d\n",
    "header_only": b">only a header",
    "header_only_newline": b">only a header\n",
    "one_empty_record": b">a\n\n",
    "lowercase_n": b">x\nacgtnnNnacgt\n",
    "iupac": b">x\nACGTRYKMSWBDHVNacgtrykmswbdhvn\n",
    "blanks": b">x\nAC GT\tAC\n \t \nN N\n",
    "gt_mid_line": b">x\nAC>GT\nA >N\n",
    "n_and_gt_in_header": b">N n >NNN> nn\nACGT\n>x N\nNA\n",
    "fastq": b"@r1 N\nACGTNN\n+\nIIIIII\n@r2\nNNA\n+r2\nIII\n",
    "fastq_crlf_no_newline": b"@r1\r\nACGTN\r\n+\r\nIIIII",
    "cutoff_odd_1_2_3": b">a\nA\n>b\nAC\n>c\nACG\n",
    "cutoff_even_2_2": b">a\nAC\n>b\nGT\n",
    "wrapped": b">w\n" + b"\n".join(SEQ[i:i + 7] for i in range(0, len(SEQ), 7)) + b"\n>v\n" + SEQ * 3 + b"\n",
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_files(tmp_path, name):
    data = EDGES[name]
    p = tmp_path / (name + ".fa")
    p.write_bytes(data)
    z = tmp_path / (name + ".fa.gz")
    z.write_bytes(gzip.compress(data))
    want = restate(data)
    for path in (p, z):
        s = ga.genome_stats([str(path)])[0]
        assert as_tuple(s) == want, path.name
        assert ga.calculate_genome_stats(str(path)) == s


def test_edge_expectations_by_hand():
    """The restatement on the cases whose answer the issue spells out."""
    assert restate(EDGES["cutoff_odd_1_2_3"]) == (3, 0, 2, 6)     # cutoff 3: 1, then 1 + 2 >= 3
    assert restate(EDGES["cutoff_even_2_2"]) == (2, 0, 2, 4)      # cutoff 2: the first 2
    assert restate(EDGES["one_empty_record"]) == (1, 0, 0, 0)     # a single empty record gives 0
    assert restate(EDGES["empty_records"]) == (4, 0, 4, 4)        # empty records count; 0 + 0 + 0 < 2 <= 4
    assert restate(EDGES["iupac"]) == (1, 2, 30, 30)              # IUPAC letters: length, only N / n ambiguous
    assert restate(EDGES["blanks"]) == (1, 2, 14, 14)             # blanks and tabs count in the length
    assert restate(EDGES["gt_mid_line"]) == (1, 1, 9, 9)          # '>' inside a line is a sequence byte
    assert restate(EDGES["n_and_gt_in_header"]) == (2, 1, 4, 6)   # header bytes never count
    assert restate(EDGES["crlf"]) == (2, 3, 9, 11)


def test_all_edges_in_one_call_any_thread_count(tmp_path, golden):
    paths, want = [], []
    for name in sorted(EDGES):
        p = tmp_path / (name + ".fa")
        p.write_bytes(EDGES[name])
        paths.append(str(p))
        want.append(restate(EDGES[name]))
    paths += golden["paths"][:6]
    one = ga.genome_stats(paths, threads=1)
    four = ga.genome_stats(paths, threads=4)
    assert [as_tuple(s) for s in one] == [as_tuple(s) for s in four]
    assert [as_tuple(s) for s in one[:len(want)]] == want


def test_file_errors_are_the_packers(tmp_path):
    good = tmp_path / "good.fa"
    good.write_bytes(b">g\nACGT\n")
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n")
    bad2 = tmp_path / "bad2.fa"
    bad2.write_bytes(b">ok\nAC\n")
    for p, status in ((empty, 3), (bad, 3), (tmp_path / "missing.fa", 2)):
        with pytest.raises(ga.GalahGpuError) as packer:
            ga.pack_files([str(good), str(p)])
        assert packer.value.status == status
        with pytest.raises(ga.GalahGpuError) as e:
            ga.genome_stats([str(good), str(p), str(bad2)])
        assert e.value.status == status
        with pytest.raises(ga.GalahGpuError):
            ga.calculate_genome_stats(str(p))
    # the lowest failing index is reported, whatever the thread count
    for threads in (1, 4):
        with pytest.raises(ga.GalahGpuError) as e:
            ga.genome_stats([str(good), str(tmp_path / "missing.fa"), str(bad), str(empty)], threads=threads)
        assert e.value.status == 2
    assert ga.genome_stats([]) == []


def test_value_type_repr_and_equality():
    a = ga.GenomeAssemblyStats(161, 6506, 8289)
    assert repr(a) == "GenomeAssemblyStats { num_contigs: 161, num_ambiguous_bases: 6506, n50: 8289 }"
    assert (a.num_contigs, a.num_ambiguous_bases, a.n50) == (161, 6506, 8289)
    # PartialEq over the reference's three fields; total_bases rides along
    assert a == ga.GenomeAssemblyStats(161, 6506, 8289, total_bases=1149523)
    assert a != ga.GenomeAssemblyStats(161, 6506, 8290)
    assert a != ga.GenomeAssemblyStats(160, 6506, 8289)
    assert a != ga.GenomeAssemblyStats(161, 6505, 8289)
    assert a != (161, 6506, 8289)
    assert repr(ga.GenomeAssemblyStats(1, 0, 1000000, 1000000)) == \
        "GenomeAssemblyStats { num_contigs: 1, num_ambiguous_bases: 0, n50: 1000000 }"


def test_abi_is_additive():
    assert ga.abi_version() == 7
    for name in ("gg_genome_stats_files", "gg_sketch_files_stats"):
        assert name in ga.EXPORTED_SYMBOLS and hasattr(ga.lib(), name)
