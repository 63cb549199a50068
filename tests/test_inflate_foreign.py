"""The device gzip inflate on DEFLATE and gzip forms that zlib's compressor
never writes (every other inflate test decodes what zlib wrote): distances
up to 32,768, header runs over the lit/len / distance boundary, a lone
distance code and none, end-of-block alone, codes of 11 to 15 bits, empty
stored and fixed blocks between dynamic ones, pigz's and libdeflate's block
shapes, every optional gzip header field; and streams a decoder must refuse
(a match reaching before its member, distance symbol 30, the unused half of
a lone distance code, an incomplete distance code).  The streams come from tests/inflate_cases.py, written
bit by bit by tests/deflate_writer.py; zlib is the reference throughout.

CPU: zlib decodes every valid stream to the text its tokens stand for and
refuses every invalid one; the DEFLATE core (tests/cpp/test_inflate_core)
does the same at every chunk / window pair, and reports from its own decode
that each stream holds what it was built for.

GPU: with GALAHGPU_INFLATE=device, sketches and lengths equal the oracle's
(zlib's gzread) and the host path's with *no batch handed back*.  The device
path checks CRC-32 and ISIZE and hands a failing batch to the host, so a
device decode defect only shows as fallbacks()["inflate_host"] going up:
that count is the assertion, under every knob set.  Invalid streams give
the host path's status and message."""
import json
import os
import subprocess
import zlib

import pytest

import galah_amd as ga
import inflate_cases as ic
import oracle
from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_inflate_core")
FAR_NAMES = ["far_fixed", "far_dynamic", "far_blocks"]
HEADER_NAMES = ["headers_" + n for n in ic.HEADER_FORMS] + ["headers_cat_" + n for n in ic.HEADER_FORMS]
INVALID_NAMES = ["before_start", "into_previous_member", "into_previous_file", "dist_code_30", "unused_half",
                 "incomplete_dist_code"]


def members_of(data):
    """zlib's text of every gzip member of data"""
    out = []
    while data:
        o = zlib.decompressobj(31)
        out.append(o.decompress(data) + o.flush())
        assert o.eof
        data = o.unused_data
    return out


def test_valid_cases_are_what_zlib_decodes():
    cases = ic.valid_cases()
    assert set(cases) - set(ic.LIBDEFLATE_NAMES) == set(ic.VALID_NAMES)
    for name, c in cases.items():
        assert [t for _, t in c.members] == members_of(c.data), name
        assert zlib.decompress(c.members[0][0], 31) == c.members[0][1], name
        # FASTA, 50 KB to 1 MB
        assert c.text[:1] == b">" and b"\n\n" not in c.text, name
        assert 50000 <= len(c.text) <= 1 << 20, name
    # all four residues of the data offset mod 4
    assert {cases["headers_fname%d" % i].info["offset"] % 4 for i in (1, 2, 3, 4)} == {0, 1, 2, 3}


def test_invalid_cases_are_refused_by_zlib():
    cases = ic.invalid_cases()
    assert list(cases) == INVALID_NAMES
    for name, c in cases.items():
        with pytest.raises(zlib.error):
            members_of(c.data)
    # the reaching member's trailer is right for the text it would make, were the reach allowed
    c = cases["into_previous_member"]
    reach, text = c.members[1]
    assert reach[-8:-4] == zlib.crc32(text).to_bytes(4, "little") and text[:100] == c.members[0][1][-100:]
    assert cases["into_previous_file"].data == reach and cases["into_previous_file"].before == c.members[0][1]


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    """Every case as a file -> {name: path}"""
    d = tmp_path_factory.mktemp("foreign")
    out = {}
    for name, c in list(ic.valid_cases().items()) + list(ic.invalid_cases().items()):
        p = d / (name + ".fna.gz")
        p.write_bytes(c.data)
        out[name] = str(p)
    prev = d / "previous.fna"  # the file into_previous_file would read from
    prev.write_bytes(ic.invalid_cases()["into_previous_file"].before)
    out["previous"] = str(prev)
    return out


@pytest.fixture(scope="module")
def core_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp")])
    return BIN


@pytest.mark.parametrize("chunk,window", [(4096, 0), (300, 0), (4096, 20000), (65536, 100000)])
def test_core_decodes_the_foreign_forms(core_binary, case_files, chunk, window):
    """The core decodes every valid case serially and as the device does, and
    says from its own decode what each held; it refuses every invalid case
    with an error status or a distance before the member's first byte."""
    valid = list(ic.valid_cases())
    paths = [case_files[n] for n in valid + INVALID_NAMES]
    r = subprocess.run([core_binary, "--chunk", str(chunk), "--window", str(window)] + paths, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(x) for x in r.stdout.splitlines()]
    assert [x["file"] for x in rows] == paths
    row = dict(zip(valid + INVALID_NAMES, rows))
    for n in valid:
        assert "refused" not in row[n] and row[n]["bytes"] == len(ic.valid_cases()[n].text), n
    for n in FAR_NAMES + HEADER_NAMES + ["hdist30_hlit286", "empties"]:
        assert row[n]["max_dist"] == 32768, n
    assert row["far_fixed"]["blocks_fixed"] == 1 and row["far_dynamic"]["blocks_dynamic"] == 1
    if chunk == 4096:
        assert row["far_blocks"]["starts_found"] > 10
    assert row["long_codes"]["max_lit_bits"] == 15 and row["long_codes"]["max_dist_bits"] == 15
    for n in ("lone_and_none_cross", "lone_and_none_per_tree"):
        assert row[n]["blocks_lone_dist"] > 0 and row[n]["blocks_no_dist"] > 0, n
    assert row["lone_and_none_cross"]["cross_runs"] > 0
    assert row["lone_and_none_per_tree"]["cross_runs"] == 0 and row["lone_and_none_per_tree"]["dist_first_rep16"] == 0
    info = ic.valid_cases()["cross_runs"].info
    assert row["cross_runs"]["cross_runs"] >= info["a"] + info["b"] and info["a"] and info["b"]
    assert row["cross_runs"]["dist_first_rep16"] >= info["c"] > 0
    e = row["empties"]
    assert e["blocks_stored"] > 10 and e["blocks_fixed"] > 3 and e["empty_blocks"] > e["blocks_stored"] + e["blocks_fixed"]
    assert row["pigz_like"]["blocks_stored"] == row["pigz_like"]["empty_blocks"] == 5
    for n in HEADER_NAMES:
        assert row[n]["members"] == (2 if "_cat_" in n else 1), n
    for n in INVALID_NAMES:
        assert "refused" in row[n] and "bytes" not in row[n], row[n]
        assert row[n]["member"] == (1 if n == "into_previous_member" else 0)
    for n in ("dist_code_30", "unused_half", "incomplete_dist_code"):
        assert row[n]["refused"] == "decode status 2"  # kDecBad
    for n in ("before_start", "into_previous_member", "into_previous_file"):
        assert row[n]["refused"] == "distance before the member's first byte"


# ---------------------------------------------------------------------------
KNOBS = {
    "default": {},
    "small_chunks_and_stage": {"GALAHGPU_GZ_CHUNK_KB": "16", "GALAHGPU_TEST_STAGE_KB": "2"},
    "decode_global": {"GALAHGPU_DECODE_GLOBAL": "1"},
    "full_areas": {"GALAHGPU_GZ_TIGHT": "0"},
    "batches_of_3": {"GALAHGPU_GZ_BATCH_FILES": "3"},
    "fake_starts": {"GALAHGPU_TEST_FAKE_STARTS": "1"},
}
ALL_KNOBS = sorted({k for v in KNOBS.values() for k in v})


def sketch(paths, mp, inflate, knobs=None, stats=False):
    """-> (sketches, lens, stats or None, fallbacks, info line) of one Context over the list"""
    for k in ALL_KNOBS:
        mp.delenv(k, raising=False)
    for k, v in (knobs or {}).items():
        mp.setenv(k, v)
    mp.setenv("GALAHGPU_INFLATE", inflate)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        if stats:
            sk, lens, st = ctx.sketch_files_stats(paths)
        else:
            (sk, lens, _), st = ctx.sketch_files(paths), None
        return sk, lens, st, ctx.fallbacks(), ctx.info_line()


@pytest.fixture(scope="module")
def reference(case_files):
    """zlib's reading of the valid list, computed once: the oracle's sketches
    (gzread) and the host inflate path's, which must agree."""
    names = list(ic.valid_cases())
    paths = [case_files[n] for n in names]
    exp_sk, exp_len = oracle.sketch_files(paths, threads=8)
    with pytest.MonkeyPatch.context() as mp:
        hsk, hl, _, _, _ = sketch(paths, mp, "host")
    assert (hl == exp_len).all()
    for g, n in enumerate(names):
        assert (hsk[g][:hl[g]] == exp_sk[g][:hl[g]]).all(), n
    return {"names": names, "paths": paths, "sk": exp_sk, "len": exp_len}


def assert_rows(ref, idx, sk, lens):
    for j, g in enumerate(idx):
        assert lens[j] == ref["len"][g], ref["names"][g]
        assert (sk[j][:lens[j]] == ref["sk"][g][:lens[j]]).all(), ref["names"][g]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_device_inflates_the_foreign_forms(reference, monkeypatch, knobs):
    """The whole valid list in one call: zlib's sketches, and nothing handed
    back -- with the CRC check that proves every byte inflated on the device.
    (The list's eight two-member files, each shorter than a search chunk,
    once cost a plan each and sent the batch to the host: inflate_host.cpp.)"""
    sk, lens, _, fb, line = sketch(reference["paths"], monkeypatch, "device", KNOBS[knobs])
    assert fb["inflate_host"] == 0, line
    assert_rows(reference, range(len(lens)), sk, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAR_NAMES + HEADER_NAMES)
def test_device_inflates_one_file_alone(reference, monkeypatch, name):
    """One file per call: its segments' and its text's offsets start at 0, so
    a ring or offset slip cannot be covered by a neighbour's bytes."""
    g = reference["names"].index(name)
    sk, lens, _, fb, line = sketch([reference["paths"][g]], monkeypatch, "device")
    assert fb["inflate_host"] == 0, line
    assert_rows(reference, [g], sk, lens)


@pytest.mark.gpu
def test_device_stats_of_the_foreign_forms(reference, monkeypatch):
    """Genome stats from the device-inflated text (a second reader of it)
    equal the host form's."""
    exp = ga.genome_stats(reference["paths"])
    sk, lens, st, fb, line = sketch(reference["paths"], monkeypatch, "device", stats=True)
    assert fb["inflate_host"] == 0, line
    assert st == exp
    assert_rows(reference, range(len(lens)), sk, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 6, 9, 12])
def test_device_inflates_libdeflate_blocks(reference, monkeypatch, level):
    """libdeflate's blocks (up to ~300 KB of text each, ~0.38 tokens per
    compressed bit from level 6 on: past the tight plan's 1/4): inflated on
    the device after the full-areas replan, nothing handed back."""
    name = "libdeflate_%d" % level
    if name not in reference["names"]:
        pytest.skip("libdeflate.so.0 does not load")
    g = reference["names"].index(name)
    sk, lens, _, fb, line = sketch([reference["paths"][g]], monkeypatch, "device")
    assert fb["inflate_host"] == 0, line
    assert_rows(reference, [g], sk, lens)
    if level >= 6:
        assert "full areas " in line and "full areas 0;" not in line, line


def status_and_message(paths, mp, inflate):
    for k in ALL_KNOBS:
        mp.delenv(k, raising=False)
    mp.setenv("GALAHGPU_INFLATE", inflate)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        try:
            sk, lens, _ = ctx.sketch_files(paths)
            return ("ok", [sk[g][:lens[g]].tolist() for g in range(len(paths))])
        except ga.GalahGpuError as e:
            return (e.status, str(e))


@pytest.mark.gpu
@pytest.mark.parametrize("name", INVALID_NAMES)
def test_device_refuses_what_zlib_refuses(case_files, monkeypatch, name):
    """Alone, and third in a list of five good files (into_previous_file
    right after the file whose last bytes its match would copy): the host
    path's status and message, naming the bad file.  The expand refuses a
    source before the unit's first byte (inflate.hip, `p < f0 + dist`), so
    the reaching members never read another member's or file's text, though
    their trailers would pass every later check if they did."""
    good = [case_files[n] for n in ("far_fixed", "headers_all", "long_codes", "empties")]
    before = case_files["previous"] if name == "into_previous_file" else good[1]
    for paths in ([case_files[name]], [good[0], before, case_files[name], good[2], good[3]]):
        host = status_and_message(paths, monkeypatch, "host")
        dev = status_and_message(paths, monkeypatch, "device")
        assert host[0] != "ok", host
        assert dev == host
        assert os.path.basename(case_files[name]) in dev[1]
        assert not any(os.path.basename(p) in dev[1] for p in paths if p != case_files[name]), dev
