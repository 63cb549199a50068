"""The pack passes of the device parser (galah_amd/csrc/parse.hip passes 1-3 and
the host scans of parse_raw_batch, multi.cpp) at every seam, on whole k-mer
sets: the cases of parse_cases.py -- 32-byte chunk, 2,048-byte wave and 8 KiB
block seams, packed-word seams, file seams in a batch, and a fuzz -- sketched
with sketch_size = 12000, where every file's sketch holds all of its k-mers,
against the reference of parse_cases.py (proved on the CPU in
test_parse_cases.py).  Plain files through GALAHGPU_PARSE=device, the same
bytes as gzip through the device inflate, a three-member context, and the
statistics passes 4 and 5, which share chunk_lines with passes 2 and 3.
Needs an MI355X."""
import pytest

import galah_amd as ga
import parse_cases as pc
from test_genome_stats import as_tuple, restate

pytestmark = pytest.mark.gpu

assert (pc.CHUNK, pc.WAVE, pc.BLOCK) == (32, 2048, 8192)  # parse.hip: kPerThread, 64 lanes of it, kBlockBytes

KINDS = [("seam", 21), ("file", 21), ("fuzz", 11), ("fuzz", 21)]
IDS = ["%s-k%d" % kk for kk in KINDS]
ENV = ("GALAHGPU_PARSE", "GALAHGPU_INFLATE", "GALAHGPU_GZ_BATCH_FILES")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(kind, k, gz) -> (cases, expected sketches, paths), written once."""
    made = {}

    def get(kind, k, gz=False):
        if (kind, k, gz) not in made:
            cases, want = pc.expected(kind, k)
            d = tmp_path_factory.mktemp("%s_k%d%s" % (kind, k, "_gz" if gz else ""))
            made[kind, k, gz] = cases, want, pc.write_cases(cases, d, gz)
        return made[kind, k, gz]
    return get


def sketch(paths, env, monkeypatch, k, **ctx_args):
    """-> sketches, lens, launches of the parse kernels, batches the inflate handed back."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    with ga.Context(k=k, sketch_size=pc.SKETCH, **ctx_args) as ctx:
        ctx.timing_enable(True)
        sk, lens, _ = ctx.sketch_files(paths)
        launches = ctx.timing_read(ga.KERNEL_PARSE)["launches"]
        handed_back = ctx.fallbacks()["inflate_host"]
    return sk, lens, launches, handed_back


def wrong_rows(cases, want, sk, lens):
    """The names of the cases whose row is not the expected sketch."""
    bad = []
    for g, (c, w) in enumerate(zip(cases, want)):
        if lens[g] != len(w) or not (sk[g][:lens[g]] == w).all():
            bad.append(c.name)
    return bad


def assert_rows(cases, want, sk, lens):
    bad = wrong_rows(cases, want, sk, lens)
    assert not bad, "%d of %d differ from the reference: %s" % (len(bad), len(cases), bad[:20])
    assert (lens < pc.SKETCH).all()  # (the observer is complete: every sketch holds all of its file's k-mers)


def orders(kind, cases, want, paths):
    """The list as it is; the file seams also reversed (other neighbours in the batch)."""
    yield cases, want, paths
    if kind == "file":
        yield cases[::-1], want[::-1], paths[::-1]


@pytest.mark.parametrize("kind,k", KINDS, ids=IDS)
def test_plain_files_device_parse(files, monkeypatch, kind, k):
    for cases, want, paths in orders(kind, *files(kind, k)):
        dsk, dl, launches, _ = sketch(paths, {"GALAHGPU_PARSE": "device"}, monkeypatch, k)
        assert launches >= 3 * -(-len(paths) // pc.BATCH_FILES)  # (passes 1-3 of every batch ran on the device)
        assert_rows(cases, want, dsk, dl)
        hsk, hl, launches, _ = sketch(paths, {"GALAHGPU_PARSE": "host"}, monkeypatch, k)
        assert launches == 0
        bad = [c.name for g, c in enumerate(cases) if hl[g] != dl[g] or not (hsk[g] == dsk[g]).all()]
        assert not bad, "%d of %d differ from the host packer: %s" % (len(bad), len(cases), bad[:20])


@pytest.mark.parametrize("kind,k", KINDS, ids=IDS)
def test_gzip_device_inflate(files, monkeypatch, kind, k):
    """Every case is one valid gzip member of FASTA text that starts with '>'
    and is not empty: inflate_batch hands none of them back."""
    env = {"GALAHGPU_INFLATE": "device"}
    if kind == "file":
        env["GALAHGPU_GZ_BATCH_FILES"] = str(pc.BATCH_FILES)  # ingest_gz.cpp batches 4,096 files: cut as the plain path's
    for cases, want, paths in orders(kind, *files(kind, k, gz=True)):
        sk, lens, launches, handed_back = sketch(paths, env, monkeypatch, k)
        assert handed_back == 0 and launches >= 3
        if kind == "file":
            assert launches >= 3 * -(-len(paths) // pc.BATCH_FILES)
        assert_rows(cases, want, sk, lens)


def test_three_members(files, monkeypatch):
    """The seam list dealt to three members in batches: the rows of one."""
    cases, want, paths = files("seam", 21)
    sk1, l1, _, _ = sketch(paths, {"GALAHGPU_PARSE": "device"}, monkeypatch, 21)
    sk3, l3, _, _ = sketch(paths, {"GALAHGPU_PARSE": "device"}, monkeypatch, 21, devices=[0, 0, 0])
    assert_rows(cases, want, sk3, l3)
    assert (l1 == l3).all() and (sk1 == sk3).all()


@pytest.mark.parametrize("kind", ["seam", "file"])
def test_statistics_passes(files, monkeypatch, kind):
    """sketch_files_stats over the same files: the statistics of
    test_genome_stats.restate, and the sketches of sketch_files bit for bit."""
    cases, want, paths = files(kind, 21)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("GALAHGPU_PARSE", "device")
    with ga.Context(k=21, sketch_size=pc.SKETCH) as ctx:
        ctx.timing_enable(True)
        sk, lens, stats = ctx.sketch_files_stats(paths)
        assert ctx.timing_read(ga.KERNEL_PARSE)["launches"] >= 4 * -(-len(paths) // pc.BATCH_FILES)
        sk0, lens0, _ = ctx.sketch_files(paths)
    assert (lens == lens0).all() and (sk == sk0).all()
    assert_rows(cases, want, sk, lens)
    bad = [(c.name, as_tuple(s), restate(c.data)) for c, s in zip(cases, stats) if as_tuple(s) != restate(c.data)]
    assert not bad, "%d of %d statistics differ: %s" % (len(bad), len(cases), bad[:5])
