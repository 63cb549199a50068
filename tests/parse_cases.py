"""FASTA files that put every seam of the device parser (galah_amd/csrc/parse.hip,
passes 1-3, and the host scans of parse_raw_batch in multi.cpp) under a
complete observer, and a reference of their own.

The observer: with sketch_size = 12000 (kMaxSketch) a file of fewer than
12,000 k-mer positions has every distinct canonical k-mer hash in its sketch,
so one wrong base, one missed or spurious break, or one header byte taken as
sequence changes the sketch.  Every case here stays under that cap by
construction (`kmer_positions`, asserted by `check_cap`): real bases are kept
to windows of about k + 60 bases next to the seam, and the rest of the file is
filler that holds no k-mer (N runs, blank lines, one long header line).

The reference: `records` restates the byte rules in parse.hip's header comment
in plain Python, not through pack.cpp; the expected sketch is
oracle.sketch_records(records(data), k, 12000).  test_parse_cases.py (CPU)
proves it against oracle.sketch_file and the host packer on every case;
test_device_parse_seams.py (GPU) holds the device passes to it.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

SKETCH = 12000  # gg_internal.hpp: kMaxSketch
CHUNK = 32      # parse.hip: kPerThread, the bytes one thread classifies
WAVE = 2048     # 64 lanes of kPerThread bytes: where block_scan and the fix ballots cross waves
BLOCK = 8192    # parse.hip: kBlockBytes, where the host scans of parse_raw_batch join the blocks
SEAMS = (CHUNK, WAVE, BLOCK, 2 * BLOCK, 3 * BLOCK)  # byte X at P - 1, byte Y at P
FILLERS = ("n", "blank", "header")
BATCH_FILES = 32  # multi.cpp: kBatchGenomes (plain files per device-parse batch)

Case = namedtuple("Case", "name data k")

# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
_SEQ = bytearray(b"N" * 256)  # every other byte breaks a k-mer
for _a, _b in zip(b"ACGTacgtUu", b"ACGTACGTTT"):
    _SEQ[_a] = _b
_SEQ = bytes(_SEQ)
_DROPPED = b" \t\r\n"  # dropped: they break nothing


def records(data):
    """The file's records as parse.hip's header comment reads them: a line that
    starts with '>' is a header (it opens a record, its bytes are no
    sequence); on every other line ACGTacgtUu are bases (case folded, U as T),
    ' ' '\\t' '\\r' '\\n' are dropped, and every other byte -- a '>' that is
    not at a line start too -- is an N."""
    assert data[:1] == b">", "a FASTA file starts with a header"
    out = []
    for line in data.split(b"\n"):
        if line[:1] == b">":
            out.append([])
        else:
            out[-1].append(line.translate(_SEQ, _DROPPED))
    return [b"".join(r) for r in out]


def kmer_positions(recs, k):
    """Sum over the runs (maximal stretches without N) of max(0, len - k + 1)."""
    return sum(max(0, len(run) - k + 1) for r in recs for run in r.split(b"N"))


def check_cap(case):
    n = kmer_positions(records(case.data), case.k)
    assert n <= SKETCH - 1, "%s: %d k-mer positions, the sketch would not hold them all" % (case.name, n)
    return n


def expected_sketch(case):
    import oracle
    return oracle.sketch_records(records(case.data), case.k, SKETCH)


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bases(rng, n):
    return _ACGT[rng.integers(0, 4, max(n, 0))].tobytes()


def _header_text(rng, n):
    """n bytes of header text (no '\\n'): stretches of 37 bases, which would be
    k-mers if they were read as sequence, with N, '>', blanks and tabs."""
    out = b""
    while len(out) < n:
        out += _bases(rng, 37) + b" N >\tACGT n>> "
    return out[:n]


def _filler(rng, kind, n):
    """n bytes without a k-mer that begin at a line start and end a line."""
    if n <= 0:
        return b""
    if kind == "header" and n >= 2:
        return b">" + _header_text(rng, n - 2) + b"\n"
    if kind == "n":
        body = (b"N" * 61 + b"\n") * (n // 62 + 1)
    else:
        body = b"   \n\n \t\n\r\n" * (n // 10 + 1)
    return body[:n - 1] + b"\n"


HEAD = b">h\n"
_AFTER = 700  # filler behind the window, then a short tail of bases


def _seam_file(name, P, kind, shape, k):
    """HEAD + filler + left | right + filler + tail, with len(HEAD + filler + left) == P."""
    rng = _rng(name)
    left, right = shape(rng, P - len(HEAD), k)
    assert len(left) <= P - len(HEAD), name
    data = HEAD + _filler(rng, kind, P - len(HEAD) - len(left)) + left
    assert len(data) == P, name
    if not right.endswith(b"\n"):
        right += b"\n"
    data += right + _filler(rng, kind, _AFTER) + _bases(rng, k + 30) + b"\n"
    return Case(name, data, k)


def _win(room, k, core=0, mod=None):
    """Bases in the window left of the seam: k + 60, or what the room allows
    beside `core` other bytes; with mod = (r, 16) the count is r mod 16."""
    n = min(k + 60, room - core)
    if mod is not None:
        n -= (n - mod) % 16
    assert n >= 0
    return n


def _simple(x, y):
    """left = bases + x, right = y + bases."""
    def shape(rng, room, k):
        return _bases(rng, _win(room, k, len(x))) + x, y + _bases(rng, k + 60)
    return shape


def _gap(nbytes):
    def shape(rng, room, k):
        gap = np.frombuffer(b"\n \r", np.uint8)[rng.integers(0, 3, nbytes)].tobytes()
        return _bases(rng, _win(room, k)), gap + _bases(rng, k + 60)
    return shape


def _long_header(length):
    def shape(rng, room, k):  # '\n' | '>': the header opens at P and holds whole blocks
        return (_bases(rng, _win(room, k, 1)) + b"\n",
                b">" + _header_text(rng, length - 2) + b"\n" + _bases(rng, k + 60))
    return shape


def _header_spans(rng, room, k):
    h = _header_text(rng, 90)
    return _bases(rng, _win(room, k, 12)) + b"\n>" + h[:10], h[10:] + b"\n" + _bases(rng, k + 60)


def _alphabet(rng, room, k):
    def mixed(n):
        b = bytearray(_bases(rng, n))
        for i in range(len(b)):
            r = int(rng.integers(0, 4))
            if b[i:i + 1] == b"T" and r < 2:
                b[i:i + 1] = b"Uu"[r:r + 1]
            elif r == 3:
                b[i:i + 1] = bytes(b[i:i + 1]).lower()
        return bytes(b)
    return mixed(_win(room, k)), mixed(k + 60)


def _before(residue):
    """`residue` mod 16 bases in front of P (the filler holds none)."""
    def shape(rng, room, k):
        n = (64 if room >= 64 + 17 else 0) + residue
        return _bases(rng, n), _bases(rng, k + 60)
    return shape


def _few_bases_block(c):
    """The BLOCK bytes from P on are c bases and then one header line: with 5
    mod 16 bases in front, the c bases share their packed word with the bases
    on both sides."""
    def shape(rng, room, k):
        return (_bases(rng, _win(room, k, mod=5)),
                _bases(rng, c) + b"\n>" + _header_text(rng, BLOCK - c - 3) + b"\n" + _bases(rng, k + 60))
    return shape


def _full_block(rng, room, k):  # 8,192 bases from packed position 15 mod 16: the ends of wl[]
    return _bases(rng, _win(room, k, mod=15)), _bases(rng, BLOCK)


def _an_block(more):
    """'AN' over BLOCK bytes (4,096 run starts, none kept) in front of P and
    `more` bytes behind it, then a run of k + 60."""
    def shape(rng, room, k):
        return (b"AN" * (BLOCK // 2))[-min(BLOCK, room):], b"AN" * (more // 2) + _bases(rng, k + 60)
    return shape


def _exact_run(extra):
    def shape(rng, room, k):  # a run of k + extra bases, half of it on each side of P
        n = k + extra
        a = min(n // 2, room - 1)
        return b"N" + _bases(rng, a), _bases(rng, n - a) + b"N"
    return shape


def _chunks_base_after_base(rng, room, k):
    """64 consecutive chunks that begin with a base after a chunk that ended
    in one, each with a run start of its own in the middle (the fix count)."""
    chunks = b"".join(_bases(rng, 15) + b"N" + _bases(rng, 16) for _ in range(64))
    return _bases(rng, _win(room, k)), chunks + _bases(rng, 20)


SHAPES = [
    # a run continues across the seam
    ("base_base", _simple(b"", b"")),
    ("base_nl_base", _simple(b"", b"\n")),
    ("nl_base", _simple(b"\n", b"")),
    # breaks at the seam
    ("base_N", _simple(b"", b"N")),
    ("N_base", _simple(b"N", b"")),
    ("N_N", _simple(b"N", b"N")),
    ("base_gt", _simple(b"", b">")),
    ("blank_gt", _simple(b" ", b">")),
    # a header at the seam
    ("nl_header", lambda rng, room, k: (_bases(rng, _win(room, k, 1)) + b"\n",
                                        b">" + _header_text(rng, 60) + b"\n" + _bases(rng, k + 60))),
    ("gt_header", lambda rng, room, k: (_bases(rng, _win(room, k, 2)) + b"\n>",
                                        _header_text(rng, 60) + b"\n" + _bases(rng, k + 60))),
    ("header_nl_base", lambda rng, room, k: (_bases(rng, _win(room, k, 5)) + b"\n>hd\n", _bases(rng, k + 60))),
    ("header_spans", _header_spans),
    ("header_block_700", _long_header(BLOCK + 700)),
    ("header_2_blocks_100", _long_header(2 * BLOCK + 100)),
    # CRLF and the alphabet
    ("cr_lf", lambda rng, room, k: (_bases(rng, _win(room, k, 1)) + b"\r",
                                    b"\n" + _bases(rng, 30) + b"\r\n" + _bases(rng, k + 30) + b"\r\n")),
    ("lower_and_u", _alphabet),
    # run-start bookkeeping
    ("an_block", _an_block(0)),
    ("an_block_chunk", _an_block(CHUNK)),
    ("an_block_wave", _an_block(WAVE)),
    ("run_k_minus_1", _exact_run(-1)),
    ("run_k", _exact_run(0)),
    ("run_k_plus_1", _exact_run(1)),
    ("chunks_base_after_base", _chunks_base_after_base),
    # word seams
    ("full_block_at_15", _full_block),
]
# a run continues across dropped bytes only (the longer gaps hold whole blocks)
SHAPES += [("gap_%d" % n, _gap(n)) for n in (1, 31, 32, WAVE, BLOCK, BLOCK + 5, 2 * BLOCK + 40)]
SHAPES += [("before_%d_mod_16" % r, _before(r)) for r in (0, 1, 15, 16, 17)]
SHAPES += [("block_of_%d_bases" % c, _few_bases_block(c)) for c in (1, 2, 3)]

DENSE_WIDTHS = (0, 31, 32, 33, 60, 2047, 2048, 2049, 8191, 8192, 8193)


def _wrap(seq, width):
    if width <= 0:
        return seq + b"\n"
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


@functools.lru_cache(maxsize=None)
def seam_cases(k=21):
    out = []
    for shape_name, shape in SHAPES:
        for P in SEAMS:
            for kind in FILLERS:
                out.append(_seam_file("%s-P%d-%s" % (shape_name, P, kind), P, kind, shape, k))
    seq = _bases(_rng("dense"), 11900)
    for w in DENSE_WIDTHS:
        out.append(Case("dense-w%d" % w, b">dense\n" + _wrap(seq, w), k))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def _sized(rng, n):
    """A file of n bytes that ends in a base, without a final newline."""
    if n <= len(HEAD):
        return HEAD[:n]
    nb = min(n - len(HEAD), 200)
    return HEAD + _filler(rng, "n", n - len(HEAD) - nb) + _bases(rng, nb)


@functools.lru_cache(maxsize=None)
def file_seam_cases(k=21):
    """The files of one call, in this order, so that they share batches: more
    than three device-parse batches of BATCH_FILES."""
    out = []
    for rep in range(3):
        rng = _rng("files%d" % rep)
        add = lambda name, data: out.append(Case("%s-r%d" % (name, rep), data, k))
        for n in (1, 2, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 16):
            add("size_%d" % n, _sized(rng, n))
            assert len(out[-1].data) == n
        for r in range(16):
            add("residue_%d" % r, _sized(rng, 96 + r))
        add("ends_in_base", b">a\n" + _bases(rng, 90))
        add("second_line_base", b">b\n" + _bases(rng, 90) + b"\n")
        add("ends_in_header", b">a\n" + _bases(rng, 60) + b"\n>" + _header_text(rng, 70))
        add("gt_alone", b">")
        add("normal_a", b">n\n" + _wrap(_bases(rng, 300), 60))
        add("header_only", b">" + _header_text(rng, 100))
        add("normal_b", b">n\n" + _wrap(_bases(rng, 300), 60))
    assert len(out) > 2 * BATCH_FILES
    return tuple(out)


FUZZ_SYMBOLS = [b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t", b"U", b"u", b"N", b">", b"\n", b"\n", b" ", b"\r",
                b"\t", b"R", b"Y"]
FUZZ_WEIGHTS = [22] * 4 + [1] * 4 + [.3, .3, 1, .6, 2, 1, .5, .3, .2, .3, .3]


@functools.lru_cache(maxsize=None)
def fuzz_cases(k):
    """200 files of fixed seeds: '>h\\n', 0 to 3 blocks of N or '\\n', then 1 to
    11,900 bytes drawn i.i.d. from FUZZ_SYMBOLS."""
    sym = np.frombuffer(b"".join(FUZZ_SYMBOLS), np.uint8)
    p = np.array(FUZZ_WEIGHTS) / sum(FUZZ_WEIGHTS)
    out = []
    for i in range(200):
        rng = np.random.default_rng(7000 + i)
        prefix = (b"N", b"\n")[int(rng.integers(0, 2))] * int(rng.integers(0, 3 * BLOCK + 1))
        body = sym[rng.choice(len(sym), int(rng.integers(1, 11901)), p=p)].tobytes()
        out.append(Case("fuzz%03d" % i, HEAD + prefix + body, k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(kind, k=21):
    """(cases, their expected sketches): computed once, shared by the tests, never changed."""
    cases = {"seam": seam_cases, "file": file_seam_cases, "fuzz": fuzz_cases}[kind](k)
    return cases, tuple(expected_sketch(c) for c in cases)


def write_cases(cases, directory, gz=False):
    """The cases as files of `directory` -> paths (gz: the same bytes as one gzip member)."""
    import gzip
    import os
    paths = []
    for i, c in enumerate(cases):
        p = os.path.join(str(directory), "%04d_%s.fa%s" % (i, c.name, ".gz" if gz else ""))
        with open(p, "wb") as f:
            f.write(gzip.compress(c.data, 6, mtime=0) if gz else c.data)
        paths.append(p)
    return paths
