"""gg_sketch_files_stats: every genome's assembly statistics from the same
read that sketches it, on each ingest path -- the host packer's record walk,
and the statistics passes of parse.hip over the batch text on the device
(GALAHGPU_PARSE=device, the device gzip inflate and its host fallback).
Compared with the fixture tests/golden/genome_stats.tsv and with the
restatement of src/genome_stats.rs in test_genome_stats.py.  Needs an MI355X."""
import gzip
import os

import numpy as np
import pytest

import galah_amd as ga
from test_genome_stats import EDGES, as_tuple, load_fixture, restate

pytestmark = pytest.mark.gpu

BLOCK = 8192  # parse.hip's kBlockBytes


@pytest.fixture(scope="module")
def plain_golden(golden, tmp_path_factory):
    """The golden genomes gunzipped (the device parser's plain-file path)."""
    d = tmp_path_factory.mktemp("plain")
    out = []
    for i, p in enumerate(golden["paths"]):
        q = d / ("g%02d.fna" % i)
        with gzip.open(p, "rb") as f:
            q.write_bytes(f.read())
        out.append(str(q))
    return out


def run(paths, env, monkeypatch, **ctx_args):
    for k in ("GALAHGPU_PARSE", "GALAHGPU_INFLATE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with ga.Context(k=21, sketch_size=1000, **ctx_args) as ctx:
        sk, lens, stats = ctx.sketch_files_stats([str(p) for p in paths])
        sk0, lens0, _ = ctx.sketch_files([str(p) for p in paths])
    assert (lens == lens0).all() and (sk == sk0).all()  # bit-identical to sketch_files on the same context
    return sk, lens, stats


PATHS = {
    "host_packer": ({"GALAHGPU_PARSE": "host"}, "plain"),
    "device_parse": ({"GALAHGPU_PARSE": "device"}, "plain"),
    "device_inflate": ({"GALAHGPU_INFLATE": "device"}, "gz"),
    "host_inflate": ({"GALAHGPU_INFLATE": "host"}, "gz"),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_golden_genomes_on_every_path(golden, plain_golden, monkeypatch, path):
    env, kind = PATHS[path]
    files = plain_golden if kind == "plain" else golden["paths"]
    fixture = load_fixture()
    sk, lens, stats = run(files, env, monkeypatch)
    for g, name in enumerate(golden["names"]):
        assert as_tuple(stats[g]) == fixture[name], name
        assert lens[g] == golden["lens"][g] and (sk[g] == golden["sketches"][g]).all(), name
    assert stats[golden["names"].index("abisko4/73.20110600_S2D.10.fna")] == ga.GenomeAssemblyStats(161, 6506, 8289)
    assert stats[golden["names"].index("set1/1mbp.fna")] == ga.GenomeAssemblyStats(1, 0, 1000000)


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def boundary_files():
    """The smallest shapes that break a wrong statistics kernel (8 KiB blocks,
    256 threads of 32 bytes), name -> bytes."""
    rng = np.random.default_rng(53)
    letters = np.frombuffer(b"ACGTNn", np.uint8)
    rnd = lambda n: letters[rng.integers(0, 4400, n) // 1000].tobytes()  # N in ~1/11, n rarely
    f = {}
    seq = rnd(40000)
    for width in (BLOCK - 1, BLOCK, BLOCK + 1):
        f["width_%d" % width] = b">w\n" + wrap(seq, width) + b">tail\n" + rnd(100) + b"\n"
    f["record_over_3_blocks"] = b">a\nAC\n>long\n" + wrap(rnd(3 * BLOCK + 500), 80) + b">b\nNN\n"
    hdr = (b"N n > NNN >> nn " * 1024)[:BLOCK + 700]  # a block starts inside this header line
    f["long_header"] = b">a\nACGTN\n>" + hdr + b"\nNNACGT\n" + b">" + hdr[:BLOCK + 9] + b"\nnA\n"
    f["3000_records"] = b">\nA\n" * 3000  # 2048 records per block: more than its threads
    f["3000_records_mixed"] = b"".join(b">\n" + b"AN"[i % 2:i % 2 + 1] * (i % 3) + b"\n" for i in range(3000))
    # N as the last byte of block 0 and as the first byte of block 1
    f["n_across_blocks"] = b">x\n" + b"A" * (BLOCK - 4) + b"NN" + b"A" * 50 + b"\n"
    # a record whose only sequence byte is the first byte of block 1
    head = b">first\n" + wrap(b"C" * 5000, 100)
    pad = BLOCK - len(head) - 3
    f["one_byte_record"] = head + b">" + b"h" * (pad - 2) + b"\n" + b">y\n" + b"N\n>z\nACGT\n"
    assert f["one_byte_record"][BLOCK:BLOCK + 1] == b"N" and f["one_byte_record"][BLOCK - 3:BLOCK] == b">y\n"
    assert f["n_across_blocks"][BLOCK - 1:BLOCK + 1] == b"NN"
    # a block boundary right after a header's '\n', and one right after its '>'
    f["header_ends_block"] = b">" + b"h" * (BLOCK - 2) + b"\n" + b"ACGTN\n"
    f["gt_ends_block"] = b">a\n" + b"G" * (BLOCK - 5) + b"\n>" + b"NNN n\nACN\n"
    assert f["gt_ends_block"][BLOCK - 1:BLOCK] == b">"
    return f


def test_block_boundary_shapes(tmp_path, monkeypatch):
    files = boundary_files()
    names = sorted(files)
    paths = []
    for n in names:
        p = tmp_path / (n + ".fa")
        p.write_bytes(files[n])
        paths.append(p)
    want = [restate(files[n]) for n in names]
    assert want[names.index("3000_records")] == (3000, 0, 1, 3000)
    assert want[names.index("n_across_blocks")][1] == 2
    _, _, dev = run(paths, {"GALAHGPU_PARSE": "device"}, monkeypatch)
    _, _, host = run(paths, {"GALAHGPU_PARSE": "host"}, monkeypatch)
    for g, n in enumerate(names):
        assert as_tuple(dev[g]) == want[g], n
        assert as_tuple(host[g]) == want[g], n


def test_no_leak_across_the_padding_between_files(tmp_path, monkeypatch):
    """6 files in one batch: the one without a final newline is followed by a
    header-only file and then a normal one."""
    data = [b">a\nACGTN\nAC\n", b">b\nNNNN\n>c\nAC\n", b">no newline\nACGTNACGT" + b"N" * 11, b">header only",
            b">normal\nAC\nGT\n", b">f\n" + b"N" * 20000 + b"\n>g\nA"]
    paths = []
    for i, d in enumerate(data):
        p = tmp_path / ("f%d.fa" % i)
        p.write_bytes(d)
        paths.append(p)
    want = [restate(d) for d in data]
    assert want[2] == (1, 12, 20, 20) and want[3] == (1, 0, 0, 0) and want[4] == (1, 0, 4, 4)
    for env in ({"GALAHGPU_PARSE": "device"}, {"GALAHGPU_PARSE": "host"}):
        _, _, stats = run(paths, env, monkeypatch)
        assert [as_tuple(s) for s in stats] == want, env


def test_edge_files_on_the_device_paths(tmp_path, monkeypatch):
    """test_genome_stats.py's edge files (CRLF, FASTQ, IUPAC, blanks, ...) through
    the packer's walk, the device parser and the device inflate (FASTQ and
    plain files there go through its host conversion)."""
    names = sorted(EDGES)
    plain, gz = [], []
    for n in names:
        p = tmp_path / (n + ".fa")
        p.write_bytes(EDGES[n])
        plain.append(p)
        z = tmp_path / (n + ".fa.gz")
        z.write_bytes(gzip.compress(EDGES[n]))
        gz.append(z)
    want = [restate(EDGES[n]) for n in names]
    for files, env in ((plain, {"GALAHGPU_PARSE": "host"}), (plain, {"GALAHGPU_PARSE": "device"}),
                       (gz, {"GALAHGPU_INFLATE": "device"}), (plain + gz, {"GALAHGPU_INFLATE": "device"})):
        _, _, stats = run(files, env, monkeypatch)
        for g, s in enumerate(stats):
            assert as_tuple(s) == want[g % len(names)], (env, names[g % len(names)])


def test_inflate_fallbacks_report_stats(tmp_path, monkeypatch):
    """Batches the device inflate hands back to the host: a multi-member gzip
    file and a CRC mismatch (the corrupt file fails the call as it does for
    sketch_files; the others' batch still gives statistics)."""
    a = b">a\n" + wrap(b"ACGTN" * 4000, 70)
    b = b">b\nNNNN\n>c\n" + wrap(b"GATTACA" * 3000, 60)
    multi = tmp_path / "multi.fa.gz"
    multi.write_bytes(gzip.compress(a) + gzip.compress(b))
    one = tmp_path / "one.fa.gz"
    one.write_bytes(gzip.compress(a))
    _, _, stats = run([multi, one], {"GALAHGPU_INFLATE": "device"}, monkeypatch)
    assert [as_tuple(s) for s in stats] == [restate(a + b), restate(a)]
    bad = bytearray(gzip.compress(b))
    bad[-8] ^= 0xFF  # the trailer's CRC-32
    crc = tmp_path / "crc.fa.gz"
    crc.write_bytes(bytes(bad))
    monkeypatch.setenv("GALAHGPU_INFLATE", "device")
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate((b"ACGTNNA" * 9, b"nnGATC", b"")))
    fqz = tmp_path / "reads.fq.gz"
    fqz.write_bytes(gzip.compress(fq))
    with ga.Context(k=21, sketch_size=1000) as ctx:
        before = ctx.fallbacks()["inflate_host"]
        _, _, stats = ctx.sketch_files_stats([str(one), str(fqz)])
        assert ctx.fallbacks()["inflate_host"] > before  # (FASTQ: the batch went back to the host threads)
        assert [as_tuple(s) for s in stats] == [restate(a), restate(fq)] and restate(fq)[:2] == (3, 20)
        with pytest.raises(ga.GalahGpuError) as e1:
            ctx.sketch_files([str(one), str(crc)])
        with pytest.raises(ga.GalahGpuError) as e2:
            ctx.sketch_files_stats([str(one), str(crc)])
        assert e1.value.status == e2.value.status == 2


def test_file_errors_as_sketch_files(tmp_path, monkeypatch):
    good = tmp_path / "good.fa"
    good.write_bytes(b">g\nACGTACGTACGTACGTACGTACGTACGT\n")
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n")
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    for mode in ("host", "device"):
        monkeypatch.setenv("GALAHGPU_PARSE", mode)
        with ga.Context(k=21, sketch_size=100) as ctx:
            for p, status in ((bad, 3), (empty, 3), (tmp_path / "missing.fa", 2)):
                with pytest.raises(ga.GalahGpuError) as e:
                    ctx.sketch_files_stats([str(good), str(p)])
                assert e.value.status == status


def test_two_members_same_results(golden, plain_golden, monkeypatch):
    for env, files in (({"GALAHGPU_PARSE": "device"}, plain_golden), ({"GALAHGPU_INFLATE": "device"}, golden["paths"]),
                       ({"GALAHGPU_PARSE": "host"}, plain_golden)):
        sk1, l1, s1 = run(files, env, monkeypatch)
        sk2, l2, s2 = run(files, env, monkeypatch, devices=[0, 0])
        assert (l1 == l2).all() and (sk1 == sk2).all()
        assert [as_tuple(s) for s in s1] == [as_tuple(s) for s in s2]


def test_cache_is_written_not_read(golden, tmp_path, monkeypatch):
    paths = golden["paths"]
    d = str(tmp_path / "cache")
    fixture = load_fixture()
    thr = ga.parse_percentage(90)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        for _ in range(2):  # (the second call finds a full cache and still reads every file)
            _, _, stats = ctx.sketch_files_stats(paths, cache_dir=d)
            assert [as_tuple(s) for s in stats] == [fixture[n] for n in golden["names"]]
        rev = list(reversed(paths))
        pairs, ani = ctx.precluster_files(rev, thr, cache_dir=d)
        assert ctx.last_cached == len(paths)
        plain, plain_ani = ctx.precluster_files(paths, thr)
    n = len(paths)
    back = sorted((n - 1 - int(p["j"]), n - 1 - int(p["i"]), int(p["common"]), int(p["total"]), float(a))
                  for p, a in zip(pairs, ani))
    assert back == [(int(p["i"]), int(p["j"]), int(p["common"]), int(p["total"]), float(a))
                    for p, a in zip(plain, plain_ani)]
    assert len(plain) == 161


def test_stats_passes_are_separate_launches(plain_golden, monkeypatch):
    """sketch_files launches the parser's three kernels per batch, as before;
    sketch_files_stats two more (counted under GG_KERNEL_PARSE)."""
    monkeypatch.setenv("GALAHGPU_PARSE", "device")
    files = plain_golden[:8]  # one batch (32 genomes at most)
    with ga.Context(k=21, sketch_size=1000) as ctx:
        ctx.timing_enable(True)
        ctx.sketch_files(files)
        assert ctx.timing_read(ga.KERNEL_PARSE)["launches"] == 3
        ctx.timing_enable(True)
        ctx.sketch_files_stats(files)
        assert ctx.timing_read(ga.KERNEL_PARSE)["launches"] == 5
        ctx.timing_enable(True)
        ctx.sketch_files(files)
        assert ctx.timing_read(ga.KERNEL_PARSE)["launches"] == 3
