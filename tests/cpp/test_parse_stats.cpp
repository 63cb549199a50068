// parse_core.hpp's assembly-statistics masks (stat_roles, record_counts: what
// parse.hip's passes 4 and 5 compute per thread) against a byte-by-byte
// restatement of the rules of src/genome_stats.rs as DESIGN.md states them:
// a record opens at a '>' that starts a line, the bytes of header lines never
// count, a record's length is its other bytes except '\n' and '\r', its
// ambiguous bases the N / n among them.  Random 32-byte chunks over an
// alphabet rich in the bytes that matter, every block limit, and every state
// of byte 0 (starts a line / on a header line / on a sequence line).
// Host only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../galah_amd/csrc/parse_core.hpp"

using namespace gg::parse;

int main() {
  std::mt19937_64 rng(12345);
  const char alphabet[] = ">>>\n\n\n\n\r\rNNnnACGTacgt \tRYKM@+-*";
  const int na = (int)sizeof(alphabet) - 1;
  const int kCases = 400000;
  for (int it = 0; it < kCases; ++it) {
    uint8_t b[32];
    // some chunks dense in line structure, some plain sequence with a few N
    const int mode = (int)(rng() % 3);
    for (int j = 0; j < 32; ++j) {
      if (mode == 0) b[j] = (uint8_t)alphabet[rng() % na];
      else if (mode == 1) b[j] = (uint8_t)(rng() % 16 == 0 ? alphabet[rng() % na] : "ACGTN"[rng() % 5]);
      else b[j] = (uint8_t)(rng() % 256);
    }
    const uint32_t lim = it % 7 == 0 ? (uint32_t)(rng() % 33) : 32u;
    const bool line0 = rng() % 3 == 0;
    const bool hdr0 = !line0 && rng() % 2 == 0;
    uint32_t w[8];
    memcpy(w, b, 32);
    const Masks m = classify(w, lim);
    const StatRoles r = stat_roles(w, m, line0, hdr0);
    // byte by byte
    uint32_t rec = 0, seq = 0, amb = 0;
    bool at_line_start = line0, in_header = hdr0;
    std::vector<uint32_t> counts(1, 0);  // [0]: the record open at byte 0, then one per record start
    for (uint32_t j = 0; j < lim; ++j) {
      const uint8_t c = b[j];
      if (at_line_start) in_header = c == '>';
      if (at_line_start && c == '>') {
        rec |= 1u << j;
        counts.push_back(0);
      }
      if (!in_header && c != '\n' && c != '\r') {
        seq |= 1u << j;
        ++counts.back();
        if (c == 'N' || c == 'n') amb |= 1u << j;
      }
      at_line_start = c == '\n';
    }
    if (r.rec != rec || r.seq != seq || r.amb != amb) {
      printf("FAIL masks at case %d: rec %08x/%08x seq %08x/%08x amb %08x/%08x\n", it, r.rec, rec, r.seq, seq, r.amb,
             amb);
      return 1;
    }
    std::vector<uint32_t> got(counts.size(), 0);
    bool ordered = true, in_range = true;
    uint32_t last_t = 0;
    record_counts(r, [&](uint32_t t, uint32_t n) {
      if (t >= got.size() || n == 0) {
        in_range = false;
        return;
      }
      if (t < last_t) ordered = false;
      last_t = t;
      got[t] += n;
    });
    if (!ordered || !in_range || got != counts) {
      printf("FAIL record_counts at case %d\n", it);
      return 1;
    }
  }
  printf("ok %d\n", kCases);
  return 0;
}
