"""A bit-level DEFLATE (RFC 1951) and gzip (RFC 1952) writer in plain Python,
for streams that zlib's compressor never writes (tests/inflate_cases.py,
tests/test_inflate_foreign.py).  Blocks are given as explicit tokens, the
Huffman code lengths of a dynamic block may be given, and the header's
run-length coding runs over the joined lit/len + distance lengths or per
tree.  Nothing here decodes: zlib is the judge of every stream.

Tokens: an int is a literal byte, (length, distance) a match.  A match's
distance may be a RawDist: a distance code written bit for bit, for streams
a decoder must refuse."""
import collections
import ctypes
import heapq
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# a distance code written as given: `nbits` bits of `code` (MSB first), then `ebits` extra bits
RawDist = collections.namedtuple("RawDist", "code nbits extra ebits")

# length 3..258 -> (lit/len symbol, extra bits, their value); 258 is symbol 285
_LEN_SYM = {}
for _i in range(28):
    for _v in range(1 << LEN_EXTRA[_i]):
        _LEN_SYM.setdefault(LEN_BASE[_i] + _v, (257 + _i, LEN_EXTRA[_i], _v))
_LEN_SYM[258] = (285, 0, 0)


def dist_symbol(dist):
    """distance 1..32768 -> (symbol, extra bits, their value)"""
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def apply(tokens, prefix=b""):
    """The text the tokens stand for (after `prefix`, which matches may reach
    into and which is not returned)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        n, d = t
        if d > len(out):
            raise ValueError("distance %d at byte %d" % (d, len(out)))
        if d >= n:
            out += out[len(out) - d:len(out) - d + n]
        else:
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(prefix):])


def kraft(lens):
    """Sum of 2^(15 - len) over the nonzero lengths (2^15: a complete code)."""
    return sum(1 << (15 - l) for l in lens if l)


def check_code(lens, limit, allow_empty):
    """The acceptance of zlib's inflate_table: a complete code, or a single
    code of length 1, or (distances only) no code at all."""
    used = [l for l in lens if l]
    assert all(1 <= l <= limit for l in used), "code length out of range"
    if not used:
        assert allow_empty, "empty code"
        return
    k = kraft(used)
    assert k == 1 << 15 or (k < 1 << 15 and max(used) == 1), "code is neither complete nor a lone length-1 code"


def lengths_from_counts(counts, limit):
    """Huffman code lengths (<= limit) for the symbols with nonzero counts.  A
    lone symbol gets length 1 and stays alone (zlib would add a second code)."""
    counts = list(counts)
    used = [s for s, c in enumerate(counts) if c]
    lens = [0] * len(counts)
    if len(used) <= 1:
        for s in used:
            lens[s] = 1
        return lens
    while True:
        heap = [(counts[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        tie = len(counts)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
            tie += 1
        if max(depth.values()) <= limit:
            break
        for s in used:  # flatter counts, a flatter tree
            counts[s] = (counts[s] + 1) // 2
    for s in used:
        lens[s] = depth[s]
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> per symbol the code with its bits reversed (so that
    it goes out LSB first like everything else)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


def run_lengths(seq, repeats=True):
    """The code-length symbols of `seq` -> [(symbol, extra value, extra bits,
    first index, lengths covered)], greedily: a nonzero value, then 16s of up
    to 6; zeros as 18s of up to 138, a 17, or single zeros."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if not repeats:
            out += [(v, 0, 0, i + r, 1) for r in range(run)]
        elif v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, 7, j - run, r))
                run -= r
            if run >= 3:
                out.append((17, run - 3, 3, j - run, run))
                run = 0
            out += [(0, 0, 0, j - run + r, 1) for r in range(run)]
        else:
            out.append((v, 0, 0, i, 1))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, 2, j - run, r))
                run -= r
            out += [(v, 0, 0, j - run + r, 1) for r in range(run)]
        i = j
    return out


class Deflate:
    """A DEFLATE stream under construction.  Everything goes out LSB first;
    Huffman codes are reversed before (RFC 1951 3.1.1).  `headers` keeps what
    each dynamic block's header held: hlit, hdist, hclen and the runs."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nbits = 0
        self.headers = []

    def bits(self, value, n):
        self.acc |= value << self.nbits
        self.nbits += n
        if self.nbits >= 64:
            self._drain()

    def _drain(self):
        k = self.nbits >> 3
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.nbits -= 8 * k

    def align(self):
        self.bits(0, -self.nbits % 8)
        self._drain()

    def bytes(self):
        """The stream so far, its last byte padded with zero bits."""
        self._drain()
        return bytes(self.out) + (bytes([self.acc]) if self.nbits else b"")

    def stored(self, data, final):
        pieces = [data[i:i + 65535] for i in range(0, len(data), 65535)] or [b""]
        for k, piece in enumerate(pieces):
            self.bits(int(bool(final) and k + 1 == len(pieces)), 1)
            self.bits(0, 2)
            self.align()
            self.out += len(piece).to_bytes(2, "little") + (len(piece) ^ 0xFFFF).to_bytes(2, "little") + piece
        return self

    def _tokens(self, tokens, lit_lens, dist_lens):
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        acc, nb = self.acc, self.nbits  # (the hot loop keeps them local)
        for t in tokens:
            if isinstance(t, int):
                assert lit_lens[t], "literal %d has no code" % t
                acc |= lc[t] << nb
                nb += lit_lens[t]
            else:
                n, d = t
                s, eb, ev = _LEN_SYM[n]
                assert lit_lens[s], "length symbol %d has no code" % s
                acc |= lc[s] << nb
                nb += lit_lens[s]
                acc |= ev << nb
                nb += eb
                if isinstance(d, RawDist):
                    acc |= int(format(d.code, "0%db" % d.nbits)[::-1], 2) << nb
                    nb += d.nbits
                    acc |= d.extra << nb
                    nb += d.ebits
                else:
                    s, eb, ev = dist_symbol(d)
                    assert dist_lens[s], "distance symbol %d has no code" % s
                    acc |= dc[s] << nb
                    nb += dist_lens[s]
                    acc |= ev << nb
                    nb += eb
            if nb >= 512:
                k = nb >> 3
                self.out += (acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
                acc >>= 8 * k
                nb -= 8 * k
        acc |= lc[256] << nb
        nb += lit_lens[256]
        self.acc, self.nbits = acc, nb
        self._drain()

    def fixed(self, tokens, final):
        self.bits(int(bool(final)), 1)
        self.bits(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)
        return self

    def dynamic(self, tokens, final, lit_lens=None, dist_lens=None, cross=True, repeats=True, hdist_min=1,
                hlit_min=257, hclen_min=4, check=True):
        """lit_lens / dist_lens: explicit code lengths per symbol (checked to
        be codes zlib accepts), else Huffman lengths from the token counts.
        cross: the run-length coding runs over the joined lit/len + distance
        sequence (a run may cover the end of one and the start of the other),
        else per tree.  hlit_min / hdist_min / hclen_min: at least that many
        lengths in the header (trailing ones zero).  check=False lets a
        code through that zlib refuses (for streams a decoder must refuse)."""
        if lit_lens is None or dist_lens is None:
            lcount, dcount = [0] * 286, [0] * 30
            lcount[256] = 1
            for t in tokens:
                if isinstance(t, int):
                    lcount[t] += 1
                else:
                    lcount[_LEN_SYM[t[0]][0]] += 1
                    if not isinstance(t[1], RawDist):
                        dcount[dist_symbol(t[1])[0]] += 1
            if lit_lens is None:
                lit_lens = lengths_from_counts(lcount, 15)
            if dist_lens is None:
                dist_lens = lengths_from_counts(dcount, 15)
        lit_lens = list(lit_lens) + [0] * (286 - len(lit_lens))
        dist_lens = list(dist_lens) + [0] * (30 - len(dist_lens))
        assert len(lit_lens) == 286 and len(dist_lens) == 30 and lit_lens[256]
        if check:
            check_code(lit_lens, 15, False)
            check_code(dist_lens, 15, True)
        hlit = max([hlit_min] + [s + 1 for s in range(286) if lit_lens[s]])
        hdist = max([hdist_min] + [s + 1 for s in range(30) if dist_lens[s]])
        if cross:
            runs = run_lengths(lit_lens[:hlit] + dist_lens[:hdist], repeats)
        else:
            runs = run_lengths(lit_lens[:hlit], repeats)
            runs += [(s, ev, eb, hlit + i, n) for s, ev, eb, i, n in run_lengths(dist_lens[:hdist], repeats)]
        ccount = [0] * 19
        for r in runs:
            ccount[r[0]] += 1
        if sum(1 for c in ccount if c) == 1:  # (zlib refuses an incomplete code-length code)
            ccount[0 if not ccount[0] else 18] += 1
        cl_lens = lengths_from_counts(ccount, 7)
        assert kraft(cl_lens) == 1 << 15
        hclen = max([hclen_min] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        self.bits(int(bool(final)), 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canonical_codes(cl_lens)
        for s, ev, eb, _, _ in runs:
            self.bits(cc[s], cl_lens[s])
            self.bits(ev, eb)
        self.headers.append({"hlit": hlit, "hdist": hdist, "hclen": hclen, "runs": runs})
        self._tokens(tokens, lit_lens, dist_lens)
        return self


def gzip_wrap(deflate_bytes, text, fname=None, comment=None, extra=None, hcrc=False, trailer_text=None):
    """One gzip member around a finished DEFLATE stream whose text is `text`.
    fname / comment: bytes without the closing zero; extra: the bytes of the
    FEXTRA field after XLEN (subfields: two id bytes, a u16 length, data);
    trailer_text: the text the trailer's CRC-32 and ISIZE are computed from,
    where it is to differ from `text`."""
    flg = (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if fname is not None else 0) | \
        (16 if comment is not None else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 255])
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if fname is not None:
        h += fname + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    t = text if trailer_text is None else trailer_text
    return h + deflate_bytes + zlib.crc32(t).to_bytes(4, "little") + (len(t) & 0xFFFFFFFF).to_bytes(4, "little")


def pigz_like(text, block=131072, level=6):
    """A gzip member shaped as pigz writes it: every `block` bytes compressed
    on their own with the 32 KB before them as the dictionary, each piece but
    the last ended by an empty stored block (Z_SYNC_FLUSH), so a piece's
    matches reach into the text of the piece before."""
    out = []
    for i in range(0, max(len(text), 1), block):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, text[max(0, i - 32768):i]) \
            if i else zlib.compressobj(level, zlib.DEFLATED, -15)
        last = i + block >= len(text)
        out.append(c.compress(text[i:i + block]) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH))
    return gzip_wrap(b"".join(out), text, fname=b"pigz_like.fna")


_LIBDEFLATE = []


def _libdeflate():
    if not _LIBDEFLATE:
        try:
            lib = ctypes.CDLL("libdeflate.so.0")
            lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
            lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
            lib.libdeflate_gzip_compress_bound.restype = ctypes.c_size_t
            lib.libdeflate_gzip_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
            lib.libdeflate_gzip_compress.restype = ctypes.c_size_t
            lib.libdeflate_gzip_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                                     ctypes.c_size_t]
            lib.libdeflate_free_compressor.restype = None
            lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
            _LIBDEFLATE.append(lib)
        except (OSError, AttributeError):
            _LIBDEFLATE.append(None)
    return _LIBDEFLATE[0]


def libdeflate_gzip(text, level):
    """`text` as a gzip member written by libdeflate's compressor, or None
    where libdeflate.so.0 does not load."""
    lib = _libdeflate()
    if lib is None:
        return None
    c = lib.libdeflate_alloc_compressor(level)
    if not c:
        return None
    try:
        cap = lib.libdeflate_gzip_compress_bound(c, len(text))
        buf = ctypes.create_string_buffer(cap)
        n = lib.libdeflate_gzip_compress(c, text, len(text), buf, cap)
        assert n, "libdeflate_gzip_compress failed"
        return buf.raw[:n]
    finally:
        lib.libdeflate_free_compressor(c)
