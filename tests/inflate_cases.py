"""Named gzip streams in forms of RFC 1951 / RFC 1952 that zlib's compressor
never writes, built with tests/deflate_writer.py from seeds (nothing is
committed compressed).  Every text is FASTA ('>' first, lines of bases with
no empty line), so the device path does not hand a file back as "not FASTA".

valid_cases()   -> {name: Case}; Case.members lists the (gzip bytes, text)
                   of each member, Case.data is the file.
invalid_cases() -> {name: Case} that zlib refuses; Case.before is the text
                   of the file to put before it in a batch (or None)."""
import functools
import gzip
import zlib

import numpy as np

import deflate_writer as dw
from deflate_writer import Deflate, RawDist

FAR_DISTS = [32768, 32767, 32766, 32513, 32507, 24577, 24576, 16385, 1, 2, 3, 4, 5]
EDGE_LENS = [3, 4, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258]


class Case:
    def __init__(self, members, before=None, info=None):
        self.members = members  # [(gzip member bytes, its text)]
        self.data = b"".join(m for m, _ in members)
        self.text = b"".join(t for _, t in members)
        self.before = before
        self.info = info or {}


class Gen:
    """FASTA text grown token by token.  Literals are bases, with a newline
    once a line has `width` of them; a match is taken only if the text stays
    free of empty lines (else a literal goes first, which moves the source)."""

    def __init__(self, seed, name=b"seq", width=70, alphabet=b"ACGT"):
        self.rng = np.random.default_rng(seed)
        self.alphabet = alphabet
        self.pool = self.alphabet_bytes(1 << 16)
        self.pi = 0
        self.width = width
        self.out = bytearray()
        self.toks = []
        for b in b">" + name + b"\n":
            self.lit(b)
        self.head = len(self.out)

    def alphabet_bytes(self, n):
        return np.frombuffer(self.alphabet, np.uint8)[self.rng.integers(0, len(self.alphabet), n)].tobytes()

    def lit(self, b):
        self.out.append(b)
        self.toks.append(b)

    def base(self):
        if self.out[-1] != 10 and len(self.out) - self.out.rfind(b"\n") > self.width:
            self.lit(10)
            return
        if self.pi == len(self.pool):
            self.pool, self.pi = self.alphabet_bytes(1 << 16), 0
        self.lit(self.pool[self.pi])
        self.pi += 1

    def bases(self, n):
        for _ in range(n):
            self.base()

    def match_ok(self, n, d):
        """May (n, d) come next?  Its source lies after the header line and
        the text gets no empty line."""
        if len(self.out) - d < self.head:
            return False
        s = len(self.out) - d
        piece = bytes(self.out[s:s + n]) if d >= n else (bytes(self.out[s:]) * (n // d + 1))[:n]
        return b"\n\n" not in bytes(self.out[-1:]) + piece and b">" not in piece

    def match(self, n, d, tries=8):
        for _ in range(tries):
            if self.match_ok(n, d):
                self.toks.append((n, d))
                s = len(self.out) - d
                for i in range(n):
                    self.out.append(self.out[s + i])
                return True
            self.base()
        return False

    def take(self):
        """The tokens since the last take (one block's)."""
        t, self.toks = self.toks, []
        return t

    def finish_line(self):
        if self.out[-1] != 10:
            self.lit(10)


def member(d, text, **kw):
    data = dw.gzip_wrap(d.bytes(), text, **kw)
    return data, text


def split_far(n):
    """n bytes as match lengths of 258 with no piece shorter than 3"""
    out = [258] * (n // 258)
    r = n % 258
    if r >= 3:
        out.append(r)
    elif r:
        out[-1:] = [130, 128 + r]
    return out


def far_case(kind):
    """32,768 bytes of literals, the same bytes again as matches of length
    258 at distance 32,768, then 20,000 more bytes the same way."""
    g = Gen(101, b"far")
    while len(g.out) < 32767:
        g.base()
    if g.out[-1] == 10:  # (the text's period ends with the one newline)
        g.out[-1] = g.toks[-1] = 65
    g.lit(10)
    assert len(g.out) == 32768
    toks = g.take() + [(n, 32768) for n in split_far(32768) + split_far(20000)]
    text = dw.apply(toks)
    assert len(text) == 32768 + 32768 + 20000 and text[32768:65536] == text[:32768]
    d = Deflate()
    if kind == "fixed":
        d.fixed(toks, True)
    else:
        d.dynamic(toks, True)
    return Case([member(d, text)])


def far_blocks_case():
    g = Gen(102, b"far_blocks")
    d = Deflate()
    g.bases(33000)
    nm = first = blocks = 0
    while len(g.out) < 340000:
        if blocks % 2 == 0 and g.match_ok(258, 32768):
            g.match(258, 32768)
            first += 1
        for i in range(3000):
            if i % 50 == 49:
                g.match(EDGE_LENS[nm % len(EDGE_LENS)], FAR_DISTS[nm % len(FAR_DISTS)])
                nm += 1
            else:
                g.base()
        d.dynamic(g.take(), False)
        blocks += 1
    g.finish_line()
    d.dynamic(g.take(), True)
    assert 3 * first >= blocks + 1, (first, blocks)
    return Case([member(d, bytes(g.out))], info={"blocks": blocks + 1, "first_far": first})


def lone_and_none_case(cross):
    """Blocks in turn without any distance code (HDIST = 1, the one length 0)
    and with matches that all use one distance symbol, whose code is then
    alone at length 1.  cross: the lit/len lengths go up to symbol 285 in
    every third block, so that a run of zeros covers the boundary."""
    g = Gen(103, b"lone_and_none")
    d = Deflate()
    lone_syms = [0, 3, 4, 9, 16, 23, 28, 29]
    b = 0
    while len(g.out) < 120000:
        if b % 2 == 0 or len(g.out) < 33000:
            g.bases(2500)
        else:
            s = lone_syms[(b // 2) % len(lone_syms)]
            for i in range(2500):
                if i % 40 == 39:
                    dist = dw.DIST_BASE[s] + (int(g.rng.integers(0, 1 << dw.DIST_EXTRA[s])) if i % 80 == 39 else
                                              (1 << dw.DIST_EXTRA[s]) - 1)
                    g.match(EDGE_LENS[(i // 40) % len(EDGE_LENS)], dist)
                else:
                    g.base()
        toks = g.take()
        d.dynamic(toks, False, cross=cross, hlit_min=286 if b % 3 == 0 else 257)
        h = d.headers[-1]
        nd = len({dw.dist_symbol(t[1])[0] for t in toks if not isinstance(t, int)})
        assert nd <= 1 and (nd == 1 or h["hdist"] == 1)
        b += 1
    g.finish_line()
    d.dynamic(g.take(), True, cross=cross)
    return Case([member(d, bytes(g.out))])


def spans(run, hlit):
    return run[3] < hlit < run[3] + run[4]


def cross_runs_case():
    """Explicit lengths, three header forms in turn: (a) a 16 whose repeats
    cover the last lit/len lengths and the first distance lengths, (b) an 18
    of zeros over the boundary, (c) a 16 as the first symbol of the distance
    part, repeating the last lit/len length."""
    g = Gen(104, b"cross_runs")
    g.finish_line()
    d = Deflate()
    d.dynamic(g.take(), False)  # (the header line's letters have no code below)
    seen = {"a": 0, "b": 0, "c": 0}

    def lit(pairs):
        lens = [0] * 286
        for s, l in pairs.items():
            lens[s] = l
        return lens

    # (a) A C G: 2, T: 3, newline and end-of-block: 5, lengths 3..6: 6 | distances 1..4: 6, then 1, 2, 3, 4
    lit_a = lit({65: 2, 67: 2, 71: 2, 84: 3, 10: 5, 256: 5, 257: 6, 258: 6, 259: 6, 260: 6})
    dist_a = [6, 6, 6, 6, 1, 2, 3, 4]
    # (c) ... newline: 4, end-of-block and length 3: 6, length 4: 5 | distances 1..4: 5, then 1, 2, 3
    lit_c = lit({65: 2, 67: 2, 71: 2, 84: 3, 10: 4, 256: 6, 257: 6, 258: 5})
    dist_c = [5, 5, 5, 5, 1, 2, 3]
    b = 0
    while len(g.out) < 90000:
        form = "abc"[b % 3]
        max_len, max_dist = {"a": (6, 16), "b": (3, 64), "c": (4, 12)}[form]
        for i in range(3000):
            if i % 25 == 24:
                n = 3 + (i // 25) % (max_len - 2)
                dist = 33 + (i // 25) % 32 if form == "b" else 1 + (i // 25) % max_dist
                g.match(n, dist)
            else:
                g.base()
        toks = g.take()
        if form == "a":
            d.dynamic(toks, False, lit_lens=lit_a, dist_lens=dist_a)
        elif form == "c":
            d.dynamic(toks, False, lit_lens=lit_c, dist_lens=dist_c)
        else:  # length 3 only and distances 33..64: zeros from symbol 258 to distance symbol 9
            d.dynamic(toks, False, hlit_min=286)
        h = d.headers[-1]
        for r in h["runs"]:
            if form == "a" and r[0] == 16 and spans(r, h["hlit"]):
                seen["a"] += 1
            if form == "b" and r[0] == 18 and spans(r, h["hlit"]):
                seen["b"] += 1
            if form == "c" and r[0] == 16 and r[3] == h["hlit"]:
                seen["c"] += 1
        b += 1
    g.finish_line()
    d.dynamic(g.take(), True)
    assert all(v >= 5 for v in seen.values()), seen
    return Case([member(d, bytes(g.out))], info=seen)


def hdist30_hlit286_case():
    """Every one of the 30 distance symbols and lit/len symbol 285 in every
    block, all 19 code-length-code fields present."""
    g = Gen(105, b"hdist30_hlit286")
    d = Deflate()
    g.bases(33000)
    d.dynamic(g.take(), False, hclen_min=19)
    while len(g.out) < 120000:
        for s in range(30):
            g.bases(60)
            top = dw.DIST_BASE[s] + (1 << dw.DIST_EXTRA[s]) - 1
            assert g.match(258 if s % 3 == 0 else EDGE_LENS[s % len(EDGE_LENS)], top if s % 2 else dw.DIST_BASE[s],
                           tries=80)
        toks = g.take()
        assert {dw.dist_symbol(t[1])[0] for t in toks if not isinstance(t, int)} == set(range(30))
        d.dynamic(toks, False, hclen_min=19)
        h = d.headers[-1]
        assert (h["hlit"], h["hdist"], h["hclen"]) == (286, 30, 19)
    g.finish_line()
    d.dynamic(g.take(), True, hclen_min=19)
    return Case([member(d, bytes(g.out))])


def long_codes_case():
    """Explicit complete codes with lengths on both sides of the device's
    one-lookup tables (10 bits): lit/len lengths 1..11, six symbols at 14 and
    four at 15; distance lengths 1..15 and a second 15.  Every symbol is
    used, the long ones in every record."""
    lit = {65: 1, 67: 2, 71: 3, 84: 4, 10: 5, 257: 6, 256: 7, 78: 8, 285: 9, 97: 10, 99: 11,
           103: 14, 116: 14, 110: 14, 62: 14, 114: 14, 101: 14, 82: 15, 89: 15, 258: 15, 270: 15}
    lit_lens = [0] * 286
    for s, l in lit.items():
        lit_lens[s] = l
    dsyms = [8, 9, 10, 11, 12, 13, 14, 15, 16, 0, 1, 20, 25, 28, 29, 3]  # lengths 1, 2, .., 15, 15
    dist_lens = [0] * 30
    for i, s in enumerate(dsyms):
        dist_lens[s] = min(i + 1, 15)
    assert dw.kraft(lit_lens) == 1 << 15 and dw.kraft(dist_lens) == 1 << 15
    g = Gen(106, b"reRY", alphabet=b"ACGT" * 12 + b"Nac")
    d = Deflate()
    used_l, used_d = set(), set()
    rec = km = 0
    while len(g.out) < 150000:
        for i in range(4000):
            if i % 500 == 250:  # another record: a header line of the rare letters
                g.finish_line()
                for b in b">reRYgtn" + b"reRYgtn"[rec % 7:]:
                    g.lit(b)
                g.lit(10)
                rec += 1
            elif i % 40 == 39 and len(g.out) > 33500:
                s = dsyms[km % len(dsyms)]
                n = [3, 4, 258, 23 + km % 4][(km // len(dsyms)) % 4]
                dist = dw.DIST_BASE[s] + (km * 7919) % (1 << dw.DIST_EXTRA[s])
                if g.match_ok(n, dist):  # (else the same one is tried again 40 tokens on)
                    g.match(n, dist)
                    km += 1
                else:
                    g.base()
            else:
                g.base()
        toks = g.take()
        for t in toks:
            if isinstance(t, int):
                used_l.add(t)
            else:
                used_l.add(dw._LEN_SYM[t[0]][0])
                used_d.add(dw.dist_symbol(t[1])[0])
        d.dynamic(toks, False, lit_lens=lit_lens, dist_lens=dist_lens)
    g.finish_line()
    d.dynamic(g.take(), True, lit_lens=lit_lens, dist_lens=dist_lens)
    assert used_l | {256} == set(lit) and used_d == set(dsyms), (set(lit) - used_l, set(dsyms) - used_d)
    return Case([member(d, bytes(g.out))])


def empty_dynamic_accepted():
    """Does zlib take a dynamic block whose only code is end-of-block, alone
    at length 1?  (zlib decides whether `empties` holds one.)"""
    d = Deflate()
    d.dynamic([], False, lit_lens=[0] * 256 + [1])
    d.stored(b"x", True)
    try:
        return zlib.decompress(d.bytes(), -15) == b"x"
    except zlib.error:
        return False


def empties_case():
    """Dynamic blocks of 4,000 tokens separated in turn by an empty stored
    block, an empty fixed block and two empty stored blocks; each block
    begins with matches into the text before the separator.  One dynamic
    block is empty (end-of-block alone at length 1); the final block is an
    empty stored one."""
    g = Gen(107, b"empties")
    d = Deflate()
    b = 0
    while len(g.out) < 160000:
        if b:
            g.match(EDGE_LENS[b % len(EDGE_LENS)], 1 + (b * 37) % 2000)
            g.base()
            if len(g.out) > 33000:
                g.match(258, FAR_DISTS[b % 5])
        for i in range(4000):
            if i % 100 == 99 and len(g.out) > 33000:
                g.match(EDGE_LENS[(i // 100) % len(EDGE_LENS)], FAR_DISTS[(i // 100) % len(FAR_DISTS)])
            else:
                g.base()
        d.dynamic(g.take(), False)
        if b % 3 == 0:
            d.stored(b"", False)
        elif b % 3 == 1:
            d.fixed([], False)
        else:
            d.stored(b"", False).stored(b"", False)
        if b == 4 and empty_dynamic_accepted():
            d.dynamic([], False, lit_lens=[0] * 256 + [1])
        b += 1
    g.finish_line()
    d.dynamic(g.take(), False)
    d.stored(b"", True)
    return Case([member(d, bytes(g.out))])


def fasta(seed, n, name, width=80):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    return b">" + name + b"\n" + b"\n".join(seq[j:j + width] for j in range(0, len(seq), width)) + b"\n"


def pigz_like_case():
    text = fasta(108, 700000, b"pigz_like")
    return Case([(dw.pigz_like(text), text)])


def header_body(seed):
    g = Gen(seed, b"headers%d" % seed)
    d = Deflate()
    g.bases(33000)
    nm = 0
    while len(g.out) < 60000:
        g.match(258, 32768)
        for i in range(2000):
            if i % 50 == 49:
                g.match(EDGE_LENS[nm % len(EDGE_LENS)], FAR_DISTS[nm % len(FAR_DISTS)])
                nm += 1
            else:
                g.base()
        d.dynamic(g.take(), False)
    g.finish_line()
    d.dynamic(g.take(), True)
    return d.bytes(), bytes(g.out)


HEADER_FORMS = {
    "fname1": dict(fname=b"a"), "fname2": dict(fname=b"ab"), "fname3": dict(fname=b"a.f"),
    "fname4": dict(fname=b"a.fa"), "comment": dict(comment=b"a comment, then the data"), "hcrc": dict(hcrc=True),
    "extra": dict(extra=b"XY\x05\x00hello"),
    "all": dict(fname=b"all.fna", comment=b"every optional field", hcrc=True, extra=b"XY\x03\x00abcZZ\x00\x00"),
}


def headers_cases():
    """One deflate body behind every optional gzip header field; each form
    alone and as the second member of a concatenation."""
    body, text = header_body(109)
    first_text = fasta(110, 60000, b"first_member")
    first = gzip.compress(first_text, 6)
    out = {}
    for name, kw in HEADER_FORMS.items():
        m = dw.gzip_wrap(body, text, **kw)
        off = len(m) - 8 - len(body)
        out["headers_" + name] = Case([(m, text)], info={"offset": off})
        out["headers_cat_" + name] = Case([(first, first_text), (m, text)], info={"offset": off})
    return out


def libdeflate_text():
    """About 680 KB with two long-range repeats spliced in"""
    t = bytearray(fasta(111, 660000, b"libdeflate"))
    a = t.index(b"\n", 200000) + 1
    piece = bytes(t[a:a + 81 * 120])  # (whole lines)
    for at in (520000, 400000):
        b = t.index(b"\n", at) + 1
        t[b:b] = piece
    return bytes(t)


@functools.lru_cache(maxsize=None)
def valid_cases():
    out = {
        "far_fixed": far_case("fixed"), "far_dynamic": far_case("dynamic"), "far_blocks": far_blocks_case(),
        "lone_and_none_cross": lone_and_none_case(True), "lone_and_none_per_tree": lone_and_none_case(False),
        "cross_runs": cross_runs_case(), "hdist30_hlit286": hdist30_hlit286_case(), "long_codes": long_codes_case(),
        "empties": empties_case(), "pigz_like": pigz_like_case(),
    }
    out.update(headers_cases())
    text = libdeflate_text()
    for level in (1, 6, 9, 12):
        data = dw.libdeflate_gzip(text, level)
        if data is not None:
            out["libdeflate_%d" % level] = Case([(data, text)])
    return out


VALID_NAMES = ["far_fixed", "far_dynamic", "far_blocks", "lone_and_none_cross", "lone_and_none_per_tree", "cross_runs",
               "hdist30_hlit286", "long_codes", "empties", "pigz_like"] + \
    ["headers_" + c + n for n in HEADER_FORMS for c in ("", "cat_")]
LIBDEFLATE_NAMES = ["libdeflate_%d" % level for level in (1, 6, 9, 12)]


@functools.lru_cache(maxsize=None)
def invalid_cases():
    out = {}
    # the first token is a match
    g = Gen(120, b"before_start")
    toks = [(3, 1)] + g.take()
    g.bases(60000)
    g.finish_line()
    d = Deflate().dynamic(toks + g.take(), True)
    out["before_start"] = Case([(dw.gzip_wrap(d.bytes(), b""), b"")])
    # a member whose first match reaches 100 bytes back, into the text before the member; the
    # trailer is computed as if that were allowed
    prev = fasta(121, 60000, b"previous")
    g = Gen(122, b"reaching")
    head = g.take()
    g.bases(60000)
    g.finish_line()
    toks = [(100, 100)] + head + g.take()
    text = dw.apply(toks, prefix=prev)
    assert text[:100] == prev[-100:]
    reaching = dw.gzip_wrap(Deflate().dynamic(toks, True).bytes(), text)
    out["into_previous_member"] = Case([(gzip.compress(prev, 6), prev), (reaching, text)])
    out["into_previous_file"] = Case([(reaching, text)], before=prev)
    # distance symbol 30 (the fixed code has one)
    g = Gen(123, b"dist_code_30")
    g.bases(30000)
    d = Deflate().dynamic(g.take(), False)
    g.bases(100)
    bad = g.take() + [(10, RawDist(30, 5, 0, 0))]
    g.bases(30000)
    g.finish_line()
    d.fixed(bad + g.take(), True)
    out["dist_code_30"] = Case([(dw.gzip_wrap(d.bytes(), b""), b"")])
    # a lone distance code (symbol 4 at length 1: the bit 0) and a match that sends the bit 1
    g = Gen(124, b"unused_half")
    g.bases(30000)
    d = Deflate().dynamic(g.take(), False)
    for i in range(2000):
        if i % 40 == 39:
            g.match(3 + i % 7, 5 + i % 2)
        else:
            g.base()
    bad = g.take() + [(5, RawDist(1, 1, 0, 1))]
    g.bases(30000)
    g.finish_line()
    d.dynamic(bad + g.take(), True)
    assert [l for l in d.headers[-1]["runs"] if l[3] >= d.headers[-1]["hlit"] and l[0] in range(1, 16)][0][0] == 1
    out["unused_half"] = Case([(dw.gzip_wrap(d.bytes(), b""), b"")])
    # a first header whose distance code is incomplete (four codes of length 6 and no other), three of
    # its lengths given by a 16 that began in the lit/len part: a header check that loses the distance
    # part of such a run, or all of the distance lengths, takes this for a block without distances
    g = Gen(125, b"x")
    g.take()
    g.bases(50000)
    lit_lens = [0] * 286
    for s, l in {65: 2, 67: 2, 71: 2, 84: 3, 10: 5, 256: 5, 257: 6, 258: 6, 259: 6, 260: 6}.items():
        lit_lens[s] = l
    d = Deflate().dynamic(g.take(), True, lit_lens=lit_lens, dist_lens=[6, 6, 6, 6], check=False)
    h = d.headers[-1]
    assert any(r[0] == 16 and spans(r, h["hlit"]) for r in h["runs"])
    out["incomplete_dist_code"] = Case([(dw.gzip_wrap(d.bytes(), b""), b"")])
    return out
