// Host test of the DEFLATE core of the device inflate
// (galah_amd/csrc/inflate_core.hpp): every gzip file given is decoded
//   (a) serially from its first block, and
//   (b) as the device does it: block starts searched every `chunk` bytes,
//       one independent decode per start (an overrun drops the start it
//       passed), tokens placed by prefix sums and back-references followed
//       to their literals,
// and both must equal zlib's output byte for byte, for every gzip member of
// the file.  Prints one JSON line per file: starts found and dropped, and
// what the core's decode saw in the stream (the longest distance and codes
// decoded, blocks per type, lone and absent distance codes, header runs over
// the lit/len / distance boundary).  A member zlib refuses must be refused
// by the core as well ("refused" in its line).  Built by tests/cpp/Makefile,
// run by tests/test_inflate.py and tests/test_inflate_foreign.py.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../galah_amd/csrc/inflate_core.hpp"

using namespace gg::inflate;

static bool read_all(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

// one gzip member (the first of gz); used receives the bytes it takes
static bool zlib_gunzip(const std::vector<uint8_t>& gz, std::vector<uint8_t>& out, size_t& used) {
  z_stream s{};
  if (inflateInit2(&s, 15 + 16) != Z_OK) return false;
  s.next_in = const_cast<uint8_t*>(gz.data());
  s.avail_in = (uInt)gz.size();
  uint8_t buf[1 << 16];
  int r;
  do {
    s.next_out = buf;
    s.avail_out = sizeof buf;
    r = inflate(&s, Z_NO_FLUSH);
    if (r != Z_OK && r != Z_STREAM_END) {
      inflateEnd(&s);
      return false;
    }
    out.insert(out.end(), buf, buf + (sizeof buf - s.avail_out));
  } while (r != Z_STREAM_END);
  used = (size_t)s.total_in;
  inflateEnd(&s);
  return true;
}

// offset of the deflate data of the gzip member at the start of gz (RFC 1952)
static long gzip_data_offset(const std::vector<uint8_t>& gz) {
  if (gz.size() < 18 || gz[0] != 0x1f || gz[1] != 0x8b || gz[2] != 8) return -1;
  const uint8_t flg = gz[3];
  size_t p = 10;
  if (flg & 4) p += 2 + (gz[p] | (gz[p + 1] << 8));
  if (flg & 8) {
    while (p < gz.size() && gz[p]) ++p;
    ++p;
  }
  if (flg & 16) {
    while (p < gz.size() && gz[p]) ++p;
    ++p;
  }
  if (flg & 2) p += 2;
  return p < gz.size() ? (long)p : -1;
}

static void expand(const std::vector<uint32_t>& toks, std::vector<uint8_t>& out) {
  for (uint32_t t : toks) {
    if (!tok_is_match(t)) {
      out.push_back((uint8_t)t);
    } else {
      const uint32_t len = tok_len(t), dist = tok_dist(t);
      const size_t from = out.size() - dist;
      for (uint32_t i = 0; i < len; ++i) out.push_back(out[from + i]);
    }
  }
}

// The device decode of one segment [s0, end) (end ~0: the file's last),
// restated serially: per block the header, then the body's sub-spans
// decoded speculatively, chained by checkpoints in rounds (a lane not right
// from its start decodes again from the true start until it meets its
// first decode) and concatenated (inflate.hip inflate_decode_kernel).
// rounds counts second-decode rounds, redo_bits the bits they decoded.
struct SpecStats {
  size_t rounds = 0, redo_bits = 0, spans = 0, span_bits = 0, windows = 0;
};
// The staged decode's window (bits of LDS stage past its word-aligned base,
// less the look-ahead): a block body longer than that is decoded in
// windows, each from the last lane's end of the one before (0: no windows,
// the global form).
static uint64_t g_window = 0;
static uint32_t spec_segment(const Bits& in, uint64_t s0, uint64_t end, uint64_t limit, LaneTables<ArrayStore>& tab,
                             ClArrays& cla, std::vector<uint32_t>& out, uint64_t& out_len, uint64_t& last_end, uint32_t& fin,
                             SpecStats& ss) {
  const bool final_seg = end == ~0ull;
  uint64_t pos = s0;
  out_len = 0;
  fin = 0;
  for (;;) {
    if (pos == end) break;
    if (pos > end || pos >= limit) {
      last_end = pos;
      return kDecOverrun;
    }
    uint64_t q = pos;
    uint32_t bf = 0, stl = 0;
    const int bt = read_block_header(in, q, tab, cla, bf, stl);
    if (bt < 0) {
      last_end = q;
      return kDecBad;
    }
    if (bt == 0) {
      if (q + 8ull * stl > limit) return kDecBad;
      for (uint32_t i = 0; i < stl; ++i) out.push_back(((const uint8_t*)in.w)[q / 8 + i]);
      out_len += stl;
      pos = q + 8ull * stl;
    } else {
      const uint64_t span_end = final_seg ? limit : end;
      uint64_t bstart = q, wbase = pos;
      bool more = true;
      while (more) {
      more = false;
      const uint64_t wend = g_window ? std::min<uint64_t>(span_end, (wbase & ~31ull) + g_window) : span_end;
      ++ss.windows;
      uint64_t L;
      uint32_t nsub;
      span_layout(bstart, wend, 64, L, nsub);
      struct Lane {
        uint64_t S, R, first = 0, Ea = 0, Eb = 0, ba = 0, bb = 0;
        uint32_t na = 0, nb = 0, sa = 0, sb = 0, nck = 0;
        int synced = -1;
        bool redone = false;
        std::vector<uint32_t> A, B;
        std::vector<uint64_t> ck;
        uint64_t E() const { return redone && synced < 0 ? Eb : Ea; }
        uint32_t st() const { return redone && synced < 0 ? sb : sa; }
      };
      std::vector<Lane> ln(nsub);
      for (uint32_t j = 0; j < nsub; ++j) {
        Lane& x = ln[j];
        x.S = bstart + j * L;
        x.R = j + 1 == nsub ? wend : x.S + L;
        x.ck.assign(span_cks(L), 0);
        x.sa = decode_span(in, x.S, x.S, x.R, tab,
                           [&](uint32_t t) {
                             if (x.A.size() >= span_cap(L)) return false;
                             x.A.push_back(t);
                             return true;
                           },
                           [&](uint32_t k, uint64_t c) {
                             if (k < x.ck.size()) x.ck[k] = c, x.nck = k + 1;
                             return true;
                           },
                           x.na, x.ba, x.Ea);
        x.first = x.nck ? x.S + ck_off(x.ck[0]) : ~0ull;
        ss.spans += 1;
        ss.span_bits += x.R - x.S;
      }
      uint32_t c_end = 0;
      bool overrun = false;
      for (;;) {
        std::vector<bool> ok(nsub);
        uint32_t c = nsub, t = nsub;
        for (uint32_t j = 0; j < nsub; ++j) {
          ok[j] = j == 0 || (ln[j - 1].st() == kSpanRange && ln[j].first == ln[j - 1].E());
          if (!ok[j] && c == nsub) c = j;
          if (ln[j].st() != kSpanRange && t == nsub) t = j;
        }
        if (t < c) {
          c_end = t;
          break;
        }
        if (c >= nsub) {
          overrun = wend == span_end;
          more = !overrun;
          c_end = nsub - 1;
          break;
        }
        ++ss.rounds;
        std::vector<uint64_t> from(nsub, ~0ull);
        for (uint32_t j = c; j < nsub; ++j)
          if (!ok[j] && ln[j - 1].st() == kSpanRange) from[j] = ln[j - 1].E();
        for (uint32_t j = c; j < nsub; ++j) {
          if (from[j] == ~0ull) continue;
          Lane& x = ln[j];
          x.B.clear();
          x.redone = true;
          x.synced = -1;
          x.first = from[j];
          x.sb = decode_span(in, from[j], x.S, x.R, tab,
                             [&](uint32_t tk) {
                               if (x.B.size() >= span_cap(L)) return false;
                               x.B.push_back(tk);
                               return true;
                             },
                             [&](uint32_t k, uint64_t cc) {
                               if (k < x.nck && ck_off(cc) == ck_off(x.ck[k])) {
                                 x.synced = (int)k;
                                 return false;
                               }
                               return true;
                             },
                             x.nb, x.bb, x.Eb);
          ss.redo_bits += x.Eb - from[j];
        }
      }
      if (overrun) {
        last_end = ln[c_end].E();
        return kDecOverrun;
      }
      if (ln[c_end].st() == kSpanBad) {
        last_end = ln[c_end].E();
        return kDecBad;
      }
      for (uint32_t j = 0; j <= c_end; ++j) {
        const Lane& x = ln[j];
        if (!x.redone) {
          out.insert(out.end(), x.A.begin() + ck_tok(x.ck[0]), x.A.begin() + x.na);
          out_len += x.ba - ck_bytes(x.ck[0]);
        } else {
          out.insert(out.end(), x.B.begin(), x.B.begin() + x.nb);
          out_len += x.bb;
          if (x.synced >= 0) {
            out.insert(out.end(), x.A.begin() + ck_tok(x.ck[x.synced]), x.A.begin() + x.na);
            out_len += x.ba - ck_bytes(x.ck[x.synced]);
          }
        }
      }
      pos = ln[c_end].E();
      bstart = wbase = pos;
      }  // (windows)
    }
    if (bf) {
      fin = 1;
      last_end = pos;
      return final_seg ? kDecOk : kDecFinalEarly;
    }
  }
  last_end = pos;
  return kDecOk;
}

// What a member's stream holds, as the core's own primitives decode it (a
// second serial walk, one symbol at a time through LaneTables::lit / dist,
// so that the length of every code decoded is seen; its tokens must equal
// decode_blocks').  A test that says it covers, say, distance 32,768 or a
// 15-bit code reads it here, from the decoder's side.
struct Features {
  uint32_t max_dist = 0, max_lit_bits = 0, max_dist_bits = 0;
  size_t blocks_stored = 0, blocks_fixed = 0, blocks_dynamic = 0;
  size_t blocks_lone_dist = 0, blocks_no_dist = 0, empty_blocks = 0;
  size_t cross_runs = 0;       // repeat codes covering the last lit/len and the first distance lengths
  size_t dist_first_rep16 = 0; // a 16 as the first symbol of the distance part
  void add(const Features& o) {
    max_dist = std::max(max_dist, o.max_dist);
    max_lit_bits = std::max(max_lit_bits, o.max_lit_bits);
    max_dist_bits = std::max(max_dist_bits, o.max_dist_bits);
    blocks_stored += o.blocks_stored;
    blocks_fixed += o.blocks_fixed;
    blocks_dynamic += o.blocks_dynamic;
    blocks_lone_dist += o.blocks_lone_dist;
    blocks_no_dist += o.blocks_no_dist;
    empty_blocks += o.empty_blocks;
    cross_runs += o.cross_runs;
    dist_first_rep16 += o.dist_first_rep16;
  }
};

// the code lengths of the dynamic header at pos, run by run
static bool header_features(const Bits& in, uint64_t pos, ClArrays& cla, Features& f) {
  const uint32_t h = in.peek(pos);
  const uint32_t hlit = ((h >> 3) & 31u) + 257u, hdist = ((h >> 8) & 31u) + 1u, hclen = ((h >> 13) & 15u) + 4u;
  uint64_t p = pos + 17;
  ClCode cl;
  if (!read_cl_code(in, p, hclen, cl, cla)) return false;
  const uint32_t n = hlit + hdist;
  uint32_t i = 0, prev = 0, nd = 0, md = 0;
  auto dist_len = [&](uint32_t at, uint32_t rep, uint32_t len) {
    const uint32_t k = at + rep > hlit ? at + rep - std::max(at, hlit) : 0;
    if (len && k) {
      nd += k;
      md = std::max(md, len);
    }
  };
  while (i < n) {
    const int s = decode_cl_sym(in, p, cl, cla);
    if (s < 0) return false;
    if (s < 16) {
      dist_len(i, 1, (uint32_t)s);
      prev = (uint32_t)s;
      ++i;
      continue;
    }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (i == 0) return false;
      rep = 3 + in.get(p, 2);
      val = prev;
      if (i == hlit) ++f.dist_first_rep16;
    } else if (s == 17) {
      rep = 3 + in.get(p, 3);
    } else {
      rep = 11 + in.get(p, 7);
    }
    if (i + rep > n) return false;
    if (i < hlit && i + rep > hlit) ++f.cross_runs;
    dist_len(i, rep, val);
    i += rep;
    if (s != 16) prev = 0;
  }
  if (nd == 0) ++f.blocks_no_dist;
  if (nd == 1 && md == 1) ++f.blocks_lone_dist;
  return true;
}

static bool features(const Bits& in, uint64_t limit_bits, LaneTables<ArrayStore>& tab, ClArrays& cla, Features& f,
                     std::vector<uint32_t>& toks) {
  uint64_t pos = 0;
  for (;;) {
    if (pos >= limit_bits) return false;
    if (((in.peek(pos) >> 1) & 3u) == 2u && !header_features(in, pos, cla, f)) return false;
    uint32_t bf = 0, stl = 0;
    const int bt = read_block_header(in, pos, tab, cla, bf, stl);
    if (bt < 0) return false;
    const size_t n0 = toks.size();
    if (bt == 0) {
      ++f.blocks_stored;
      for (uint32_t i = 0; i < stl; ++i) toks.push_back(in.get(pos, 8));
    } else {
      ++(bt == 1 ? f.blocks_fixed : f.blocks_dynamic);
      Cursor cur{in.w};
      cur.seek(pos);
      for (;;) {
        if (cur.pos >= limit_bits) return false;
        uint64_t p0 = cur.pos;
        const int sy = tab.lit(cur);
        if (sy < 0) return false;
        f.max_lit_bits = std::max(f.max_lit_bits, (uint32_t)(cur.pos - p0));
        if (sy < 256) {
          toks.push_back((uint32_t)sy);
          continue;
        }
        if (sy == 256) break;
        const uint32_t li = (uint32_t)sy - 257u;
        if (li >= 29) return false;
        const uint32_t len = len_base(li) + cur.get(len_extra(li));
        p0 = cur.pos;
        const int d = tab.dist(cur);
        if (d < 0 || d >= 30) return false;
        f.max_dist_bits = std::max(f.max_dist_bits, (uint32_t)(cur.pos - p0));
        const uint32_t dist = dist_base((uint32_t)d) + cur.get(dist_extra((uint32_t)d));
        f.max_dist = std::max(f.max_dist, dist);
        toks.push_back(tok_match(len, dist));
      }
      pos = cur.pos;
    }
    if (toks.size() == n0) ++f.empty_blocks;
    if (bf) return true;
  }
}

// A member zlib refuses: the core must refuse it too -- its serial decode
// ends with an error status, or a match reaches before the member's first
// byte (the test the device's expand makes on every match, inflate.hip) --
// and not hand out text.  Returns the reason, or "" if the core decodes it.
static std::string core_refusal(const Bits& in, uint64_t limit_bits, LaneTables<ArrayStore>& tab, ClArrays& cla) {
  std::vector<uint32_t> toks;
  uint64_t out_len = 0, last_end = 0;
  uint32_t bf = 0;
  const uint32_t st = decode_blocks(in, 0, ~0ull, limit_bits, tab, cla,
                                    [&](uint32_t t) {
                                      toks.push_back(t);
                                      return true;
                                    },
                                    out_len, last_end, bf);
  if (st != kDecOk) return "decode status " + std::to_string(st);
  uint64_t at = 0;
  for (uint32_t t : toks) {
    if (tok_is_match(t) && tok_dist(t) > at) return "distance before the member's first byte";
    at += tok_len(t);
  }
  return "";
}

int main(int argc, char** argv) {
  int failures = 0;
  uint32_t chunk = 4096;
  int first = 1;
  for (;;) {
    if (argc > first + 1 && std::string(argv[first]) == "--chunk") {
      chunk = (uint32_t)atoi(argv[first + 1]);
      first += 2;
    } else if (argc > first + 1 && std::string(argv[first]) == "--window") {
      g_window = (uint64_t)atoll(argv[first + 1]);
      first += 2;
    } else {
      break;
    }
  }
  // One gzip member (gz from its first byte to the file's end, `used` bytes
  // of it the member; want: zlib's text of it), its counts added to the file's row.  false: it failed.
  struct Row {
    size_t bytes = 0, found = 0, dropped = 0, lanes = 0, tokens = 0, max_chain = 0, match_bytes = 0, marker_bytes = 0,
           marker_groups = 0, members = 0;
    SpecStats ss;
    Features ft;
  };
  auto member = [&](const char* name, const std::vector<uint8_t>& gz, size_t used, const std::vector<uint8_t>& want,
                    Row& row) {
    const long off = gzip_data_offset(gz);
    const size_t nbytes = used - (size_t)off - 8;  // (its deflate data: up to the trailer)
    std::vector<uint32_t> words((nbytes + 3) / 4 + 1024, 0);  // (a header walk may read ~4.5 kbit past the end)
    memcpy(words.data(), gz.data() + off, nbytes);
    const Bits in{words.data()};
    const uint64_t limit_bits = (uint64_t)nbytes * 8;
    LaneTables<ArrayStore> tab;
    ClArrays cla;
    // (a) serially
    std::vector<uint32_t> toks;
    uint64_t out_len = 0, last_end = 0;
    uint32_t bf = 0;
    const uint32_t st = decode_blocks(in, 0, ~0ull, limit_bits, tab, cla,
                                      [&](uint32_t t) {
                                        toks.push_back(t);
                                        return true;
                                      },
                                      out_len, last_end, bf);
    std::vector<uint8_t> got;
    expand(toks, got);
    if (st != kDecOk || got != want || out_len != want.size()) {
      fprintf(stderr, "%s: serial decode differs (status %u, %zu vs %zu bytes)\n", name, st, got.size(), want.size());
      ++failures;
      return false;
    }
    // (b) as the device: starts, independent decodes, place + resolve
    std::vector<uint64_t> starts{0};
    for (uint64_t c = chunk; c < nbytes; c += chunk) {
      for (uint64_t p = c * 8; p < std::min<uint64_t>((c + chunk) * 8, limit_bits); ++p) {
        uint64_t q = p;
        SeqBits sb{Cursor{in.w}};
        sb.c.seek(p);
        uint64_t q2 = p;
        const bool ok2 = block_header_ok(sb, q2, cla);  // (the device's cursor reader)
        const bool ok1 = block_header_ok(in, q, cla);
        if (ok1 != ok2 || (ok1 && q != q2)) {
          fprintf(stderr, "%s: header check through SeqBits differs at bit %llu\n", name, (unsigned long long)p);
          ++failures;
        }
        // the search's stepwise walk (HeaderWalk) gives the same verdict
        HeaderWalk hw;
        int v = hw.start(in, p, cla) ? 0 : -1;
        while (v == 0) v = hw.step(in, cla);
        if ((v == 1) != ok1) {
          fprintf(stderr, "%s: HeaderWalk differs from block_header_ok at bit %llu\n", name, (unsigned long long)p);
          ++failures;
        }
        if (ok1) {
          starts.push_back(p);
          break;
        }
      }
    }
    const size_t found = starts.size();
    size_t dropped = 0;
    std::vector<std::vector<uint32_t>> part;
    std::vector<uint64_t> part_len;
    for (;;) {  // drop the starts a lane overran, until every lane lands
      part.assign(starts.size(), {});
      part_len.assign(starts.size(), 0);
      bool again = false;
      for (size_t b = 0; b < starts.size() && !again; ++b) {
        const uint64_t end = b + 1 < starts.size() ? starts[b + 1] : ~0ull;
        uint64_t ol, le;
        uint32_t fin;
        const uint32_t r = decode_blocks(in, starts[b], end, limit_bits, tab, cla,
                                         [&](uint32_t t) {
                                           part[b].push_back(t);
                                           return true;
                                         },
                                         ol, le, fin);
        part_len[b] = ol;
        if (r == kDecOverrun) {
          starts.erase(starts.begin() + (long)b + 1);
          ++dropped;
          again = true;
        } else if (r != kDecOk) {
          fprintf(stderr, "%s: lane %zu status %u\n", name, b, r);
          ++failures;
          starts.clear();
          break;
        }
      }
      if (!again) break;
    }
    if (starts.empty()) return false;
    // (c) the device decode of each lane's segment: the same tokens
    SpecStats ss;
    for (size_t b = 0; b < starts.size(); ++b) {
      const uint64_t end = b + 1 < starts.size() ? starts[b + 1] : ~0ull;
      std::vector<uint32_t> t3;
      uint64_t ol, le;
      uint32_t fin;
      const uint32_t r = spec_segment(in, starts[b], end, limit_bits, tab, cla, t3, ol, le, fin, ss);
      if (r != kDecOk || t3 != part[b] || ol != part_len[b]) {
        fprintf(stderr, "%s: lane %zu: sub-span decode differs (status %u, %zu vs %zu tokens)\n", name, b, r,
                t3.size(), part[b].size());
        ++failures;
        starts.clear();
        break;
      }
    }
    if (starts.empty()) return false;
    // place: every byte a literal (bit 31) or a pointer to an earlier byte
    std::vector<uint32_t> val;
    // (stats: bytes copied by matches, and the bytes the device's expand
    // leaves to the resolve pass -- a copy whose source, followed inside its
    // segment, lies before the segment -- and the 16-byte groups holding one)
    std::vector<uint8_t> marker;
    size_t match_bytes = 0;
    for (size_t b = 0; b < part.size(); ++b) {
      const size_t o0 = val.size();
      for (uint32_t t : part[b]) {
        if (!tok_is_match(t)) {
          val.push_back(0x80000000u | t);
          marker.push_back(0);
        } else {
          const uint32_t len = tok_len(t), dist = tok_dist(t);
          const size_t at = val.size();
          for (uint32_t i = 0; i < len; ++i) {
            const size_t src = at + i - dist;
            val.push_back((uint32_t)src);
            marker.push_back(src < o0 || marker[src] ? 1 : 0);
          }
          match_bytes += len;
        }
      }
    }
    size_t marker_bytes = 0, marker_groups = 0;
    for (size_t g = 0; g * 16 < marker.size(); ++g) {
      size_t m = 0;
      for (size_t i = g * 16; i < std::min(marker.size(), g * 16 + 16); ++i) m += marker[i];
      marker_bytes += m;
      marker_groups += m ? 1 : 0;
    }
    std::vector<uint8_t> got2(val.size());
    size_t max_chain = 0;
    for (size_t i = 0; i < val.size(); ++i) {
      uint32_t v = val[i];
      size_t chain = 0;
      while (!(v >> 31)) {
        v = val[v];
        ++chain;
      }
      max_chain = std::max(max_chain, chain);
      got2[i] = (uint8_t)v;
    }
    if (got2 != want) {
      fprintf(stderr, "%s: chunked decode differs\n", name);
      ++failures;
      return false;
    }
    // what the stream held, seen by the core (the same tokens, symbol by symbol)
    Features ft;
    std::vector<uint32_t> toks2;
    if (!features(in, limit_bits, tab, cla, ft, toks2) || toks2 != toks) {
      fprintf(stderr, "%s: the symbol-by-symbol walk differs from decode_blocks\n", name);
      ++failures;
      return false;
    }
    row.bytes += want.size();
    row.found += found;
    row.dropped += dropped;
    row.lanes += starts.size();
    row.tokens += toks.size();
    row.max_chain = std::max(row.max_chain, max_chain);
    row.match_bytes += match_bytes;
    row.marker_bytes += marker_bytes;
    row.marker_groups += marker_groups;
    row.ss.rounds += ss.rounds;
    row.ss.spans += ss.spans;
    row.ss.span_bits += ss.span_bits;
    row.ss.redo_bits += ss.redo_bits;
    row.ss.windows += ss.windows;
    row.ft.add(ft);
    ++row.members;
    return true;
  };
  for (int a = first; a < argc; ++a) {
    std::vector<uint8_t> file;
    if (!read_all(argv[a], file) || gzip_data_offset(file) < 0) {
      fprintf(stderr, "%s: unreadable\n", argv[a]);
      ++failures;
      continue;
    }
    // every gzip member in turn (counts summed over them, starts searched per member)
    Row row;
    bool ok = true;
    size_t at = 0;
    while (ok && at + 18 <= file.size() && file[at] == 0x1f && file[at + 1] == 0x8b) {
      const std::vector<uint8_t> gz(file.begin() + (long)at, file.end());
      std::vector<uint8_t> want;
      size_t used = 0;
      const long off = gzip_data_offset(gz);
      if (off < 0) {
        fprintf(stderr, "%s: unreadable\n", argv[a]);
        ++failures;
        ok = false;
      } else if (!zlib_gunzip(gz, want, used)) {
        // zlib refuses this member: so must the core
        const size_t nbytes = gz.size() - (size_t)off;
        std::vector<uint32_t> words((nbytes + 3) / 4 + 1024, 0);
        memcpy(words.data(), gz.data() + off, nbytes);
        LaneTables<ArrayStore> tab;
        ClArrays cla;
        const Bits in{words.data()};
        const std::string why = core_refusal(in, (uint64_t)nbytes * 8, tab, cla);
        // the search's two header checks agree on the member's first header, refused or not
        uint64_t q = 0;
        const bool ok1 = block_header_ok(in, q, cla);
        HeaderWalk hw;
        int v = hw.start(in, 0, cla) ? 0 : -1;
        while (v == 0) v = hw.step(in, cla);
        if ((v == 1) != ok1) {
          fprintf(stderr, "%s: HeaderWalk differs from block_header_ok at the member's first bit\n", argv[a]);
          ++failures;
        }
        if (why.empty()) {
          fprintf(stderr, "%s: member %zu: zlib refuses it, the core decodes it\n", argv[a], row.members);
          ++failures;
        } else {
          printf("{\"file\": \"%s\", \"refused\": \"%s\", \"member\": %zu}\n", argv[a], why.c_str(), row.members);
        }
        ok = false;
      } else {
        ok = member(argv[a], gz, used, want, row);
        at += used;
      }
    }
    if (!ok) continue;
    const SpecStats& ss = row.ss;
    const Features& ft = row.ft;
    printf("{\"file\": \"%s\", \"bytes\": %zu, \"gz_bytes\": %zu, \"starts_found\": %zu, \"starts_dropped\": %zu, "
           "\"lanes\": %zu, \"tokens\": %zu, \"max_chain\": %zu, \"redo_rounds\": %zu, \"spans\": %zu, \"span_bits\": %zu, \"redo_bits\": %zu, \"windows\": %zu, "
           "\"match_bytes\": %zu, \"marker_bytes\": %zu, \"marker_groups\": %zu, \"members\": %zu, "
           "\"max_dist\": %u, \"max_lit_bits\": %u, \"max_dist_bits\": %u, \"blocks_stored\": %zu, \"blocks_fixed\": %zu, "
           "\"blocks_dynamic\": %zu, \"blocks_lone_dist\": %zu, \"blocks_no_dist\": %zu, \"empty_blocks\": %zu, "
           "\"cross_runs\": %zu, \"dist_first_rep16\": %zu}\n",
           argv[a], row.bytes, file.size(), row.found, row.dropped, row.lanes, row.tokens, row.max_chain, ss.rounds,
           ss.spans, ss.span_bits, ss.redo_bits, ss.windows, row.match_bytes, row.marker_bytes, row.marker_groups,
           row.members, ft.max_dist, ft.max_lit_bits, ft.max_dist_bits, ft.blocks_stored, ft.blocks_fixed,
           ft.blocks_dynamic, ft.blocks_lone_dist, ft.blocks_no_dist, ft.empty_blocks, ft.cross_runs,
           ft.dist_first_rep16);
  }
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  return 0;
}
