"""The seam cases of parse_cases.py and their reference, proved without a GPU:
every case stays under the k-mer cap that makes a sketch of 12,000 a complete
observer; parse_cases.records (the byte rules restated) gives the sketch that
oracle.sketch_file gives on the file itself; and the host packer's runs
(gg_pack_files, pack.cpp) give it too, which pins pack.cpp on the same shapes.
The device passes are held to the same expectation in
test_device_parse_seams.py (GPU)."""
import os

import numpy as np
import pytest

import galah_amd as ga
import oracle
import parse_cases as pc
from conftest import ROOT
from test_host import packed_records

KINDS = [("seam", 21), ("file", 21), ("fuzz", 11), ("fuzz", 21)]
IDS = ["%s-k%d" % kk for kk in KINDS]


def test_the_restatement_by_hand():
    recs = pc.records(b">h ACGT\nAC gt\r\nUuN>\tx\n\n>\n>two >\n >A\nC")
    assert recs == [b"ACGTTTNNN", b"", b"NAC"]
    assert pc.kmer_positions(recs, 3) == 4 and pc.kmer_positions(recs, 7) == 0
    assert pc.kmer_positions([b"ACGTNACGTA", b"AC"], 4) == 1 + 2


def test_every_seam_has_its_bytes():
    """The seam sits where the case's name says, deep in the file."""
    by_name = {c.name: c.data for c in pc.seam_cases()}
    assert len(by_name) == len(pc.SHAPES) * len(pc.SEAMS) * len(pc.FILLERS) + len(pc.DENSE_WIDTHS)
    seq = b"ACGTacgtUu"
    for P in pc.SEAMS:
        for kind in pc.FILLERS:
            at = lambda shape: by_name["%s-P%d-%s" % (shape, P, kind)][P - 1:P + 1]
            d = by_name["base_base-P%d-%s" % (P, kind)]
            assert d[P - 1] in seq and d[P] in seq
            assert at("base_nl_base")[1:] == b"\n" and at("nl_base")[:1] == b"\n"
            assert at("base_N")[1:] == b"N" and at("N_base")[:1] == b"N" and at("N_N") == b"NN"
            assert at("base_gt")[1:] == b">" and at("blank_gt") == b" >"
            assert at("nl_header") == b"\n>" and at("gt_header")[:1] == b">" and at("header_nl_base")[:1] == b"\n"
            assert at("cr_lf") == b"\r\n"
            for shape, length in (("header_block_700", pc.BLOCK + 700), ("header_2_blocks_100", 2 * pc.BLOCK + 100)):
                d = by_name["%s-P%d-%s" % (shape, P, kind)]
                assert d[P:P + 1] == b">" and d.find(b"\n", P) == P + length - 1
            d = by_name["header_spans-P%d-%s" % (P, kind)]
            assert d.rfind(b"\n>", 0, P) == P - 12 and d.find(b"\n", P) == P + 80
            d = by_name["gap_%d-P%d-%s" % (2 * pc.BLOCK + 40, P, kind)]
            assert not d[P:P + 2 * pc.BLOCK + 40].strip(b"\n \r") and d[P - 1] in seq and d[P + 2 * pc.BLOCK + 40] in seq
            for c in (1, 2, 3):
                d = by_name["block_of_%d_bases-P%d-%s" % (c, P, kind)]
                assert d[P + c:P + c + 2] == b"\n>" and d.find(b"\n", P + c + 1) == P + pc.BLOCK - 1
            d = by_name["full_block_at_15-P%d-%s" % (P, kind)]
            assert not d[P:P + pc.BLOCK].strip(b"ACGT") and d[P + pc.BLOCK:P + pc.BLOCK + 1] == b"\n"
            d = by_name["an_block-P%d-%s" % (P, kind)]
            n = min(pc.BLOCK, P - len(pc.HEAD))
            assert d[P - n:P] == (b"AN" * pc.BLOCK)[-n:] and d[P] in seq


def test_file_seam_sizes():
    cases = pc.file_seam_cases()
    with open(os.path.join(ROOT, "galah_amd", "csrc", "multi.cpp")) as f:
        assert "constexpr uint32_t kBatchGenomes = %d;" % pc.BATCH_FILES in f.read()
    assert len(cases) > 2 * pc.BATCH_FILES
    sizes = [len(c.data) for c in cases]
    for n in (1, 2, 15, 16, 17, 8191, 8192, 8193, 16384, 16400):
        assert n in sizes
    assert {n % 16 for n in sizes if 96 <= n < 112} == set(range(16))


@pytest.mark.parametrize("kind,k", KINDS, ids=IDS)
def test_cap_and_the_three_references(tmp_path, kind, k):
    cases, want = pc.expected(kind, k)
    paths = pc.write_cases(cases, tmp_path)
    total = 0
    for c, p, w in zip(cases, paths, want):
        assert c.k == k and c.data[:1] == b">"
        total += pc.check_cap(c)
        assert len(w) < pc.SKETCH, c.name
        got = oracle.sketch_file(p, k, pc.SKETCH)
        assert len(got) == len(w) and (got == w).all(), c.name
    print("%s k=%d: %d files, %d k-mer positions" % (kind, k, len(cases), total))
    assert total > 100 * len(cases) or kind == "file"
    pk = ga.pack_files(paths, k)
    for c, runs, w in zip(cases, packed_records(pk), want):
        assert all(len(r) >= k for r in runs), c.name
        got = oracle.sketch_records(runs, k, pc.SKETCH) if runs else np.zeros(0, np.uint64)
        assert len(got) == len(w) and (got == w).all(), c.name
