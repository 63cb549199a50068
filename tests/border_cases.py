"""Inputs of the border-form tests and a numpy model of the border schedule
(galah_amd/csrc/matrix_core.hpp, "the border form").  Used by
test_border_schedule.py on the CPU, which keeps the model honest against the
host merge and pins what every scenario must contain, and by
test_pairs_border_matrix_gpu.py on the GPU.

The model restates, for rows 0 .. n-1 of which the last n_new = n - n_old are
new: the positions (new rows first), the border column rule (a hash held at
two or more positions, one of them new), the border tile pairs in workgroup
order and the visited cells; the chunk loop of a tile pair is matrix_cases'.
"""
import functools

import numpy as np

import matrix_cases as mc

TILE = mc.TILE
CHUNK = mc.CHUNK


def border_rows(n, n_old):
    """matrix::border_row_of for every position: the new rows first."""
    return list(range(n_old, n)) + list(range(n_old))


def border_tile_pairs(n, n_old):
    """The border tile pairs in workgroup order: the triangle over the new
    tiles (tile_pair_of), then the rectangle, tj outer."""
    t, tn = -(-n // TILE), -(-(n - n_old) // TILE)
    tri = [(ti, tj) for tj in range(tn) for ti in range(tj + 1)]
    return tri + [(ti, tj) for tj in range(tn, t) for ti in range(tn)]


def border_columns(sk, lens, n_old):
    """The border column rule -> (pieces by position, n_columns,
    column_entries, new_entries, old_only_columns)."""
    n = len(lens)
    n_new = n - n_old
    held = [sk[r, :lens[r]] for r in border_rows(n, n_old)]
    if not sum(len(h) for h in held):
        return [np.zeros(0, np.int64) for _ in held], 0, 0, 0, 0
    u, inv, cnt = np.unique(np.concatenate(held), return_inverse=True, return_counts=True)
    new_cnt = np.zeros(len(u), np.int64)
    np.add.at(new_cnt, inv[:sum(len(h) for h in held[:n_new])], 1)
    keep = (cnt >= 2) & (new_cnt >= 1)
    ids = np.cumsum(keep) - 1
    pieces, at = [], 0
    for h in held:
        i = inv[at:at + len(h)]
        at += len(h)
        pieces.append(ids[i[keep[i]]].astype(np.int64))
    return (pieces, int(keep.sum()), int(cnt[keep].sum()), int(new_cnt[keep].sum()),
            int(((cnt >= 2) & (new_cnt == 0)).sum()))


def dict_border_columns(sk, lens, n_old):
    """(columns, column entries) of the border from a dict, without the model."""
    held = {}
    for r in range(len(lens)):
        for h in sk[r, :lens[r]].tolist():
            c = held.setdefault(h, [0, 0])
            c[0] += 1
            c[1] += r >= n_old
    kept = [c for c in held.values() if c[0] >= 2 and c[1] >= 1]
    return len(kept), sum(c[0] for c in kept)


def exact_index_reads(sk, lens, n_old):
    """The member reads of the index border kernel: every entry of a new row
    reads the members before it (the rows that hold the hash, ascending)."""
    seen, reads = {}, 0
    for r in range(len(lens)):
        for h in sk[r, :lens[r]].tolist():
            if r >= n_old:
                reads += seen.get(h, 0)
            seen[h] = seen.get(h, 0) + 1
    return reads


def index_reads_bound(n_columns, column_entries, new_entries):
    """matrix::border_index_reads."""
    if not n_columns:
        return 0
    return (column_entries - new_entries) + (new_entries * new_entries // n_columns - new_entries) // 2


class BorderSchedule:
    """pieces, the counts, and pairs[(ti, tj)] a matrix_cases.TilePair for
    every border tile pair, in workgroup order (self.order)."""

    def __init__(self, sk, lens, n_old):
        self.n, self.n_old, self.n_new = len(lens), n_old, len(lens) - n_old
        self.rows = border_rows(self.n, n_old)
        self.lens = [int(lens[r]) for r in self.rows]
        self.pieces, self.n_columns, self.column_entries, self.new_entries, self.old_only_columns = \
            border_columns(sk, lens, n_old)
        self.order = border_tile_pairs(self.n, n_old) if self.n >= 2 else []
        self.pairs = {k: mc.TilePair(self.pieces, self.n, *k) for k in self.order}
        self.tiles_new = -(-self.n_new // TILE)

    def visited(self, pa, pb):
        return pa < pb and pa < self.n_new

    def common(self):
        """{(i, j): common} of every visited cell, row indices i < j, from the chunks that were run."""
        out = {}
        for (ti, tj), p in self.pairs.items():
            c = p.common
            for x, pa in enumerate(p.a):
                for y, pb in enumerate(p.b):
                    if self.visited(pa, pb):
                        i, j = sorted((self.rows[pa], self.rows[pb]))
                        assert (i, j) not in out
                        out[(i, j)] = int(c[x, y]) if self.lens[pa] and self.lens[pb] else 0
        return out

    # ---- what a scenario must contain ----
    def ends_without_a_chunk(self):
        """Tile pairs of an old tile whose pieces are all empty: no search finds an id, no chunk is run."""
        return [k for k, p in self.pairs.items()
                if k[1] >= self.tiles_new and not p.events and all(len(self.pieces[b]) == 0 for b in p.b)]

    def jumps_then_runs(self):
        return [k for k, p in self.pairs.items() if p.kinds().startswith("jr") and p.common.any()]

    def mixed_row(self):
        """Tile pairs of the tile row that holds new and old positions, with cells the visited rule skips."""
        if self.n_new % TILE == 0:
            return []
        ti = self.n_new // TILE
        return [k for k in self.order if k[0] == ti]


# ---- the scenarios ------------------------------------------------------------------------
J_HOMES = (1, 26)
J_EXTRAS = (5, 6, 7, 8, 9, 19, 20, 21, 22, 23)
J_N_OLD, J_N = 280, 300


@functools.lru_cache(maxsize=None)
def scenario_jumps():
    """28 clusters of 10 rows at s = 64 in cluster order (matrix_cases'
    banded clusters): 280 old rows, then 20 new rows -- ten drawn from
    cluster 1's pool and ten from cluster 26's, 24 hashes each, and 40 hashes
    of one other cluster (new rows 2 x and 2 x + 1 take the two halves of the
    first 80 hashes of cluster J_EXTRAS[x]'s pool).  The border's columns are
    the hashes of the touched clusters only, in cluster order: about 90 of
    cluster 1, 400 of clusters 5 .. 9, 400 of 19 .. 23, 90 of 26.  Positions:
    the 20 new rows, then the old rows; tile 2 (old rows 108 .. 171, clusters
    10 .. 17) holds no column at all, tile 4 (clusters 23 .. 27) none below
    512 -> (sk, lens, n_old)."""
    sk, lens = mc.banded_clusters(28, 10, 64, seed=7)
    rng = np.random.default_rng(8)
    new = np.zeros((20, 64), np.uint64)
    for i in range(20):
        home = mc.cluster_pool(J_HOMES[i // 10], 64)
        extra = mc.cluster_pool(J_EXTRAS[i // 2], 64)[40 * (i % 2):40 * (i % 2) + 40]
        new[i] = np.sort(np.concatenate([rng.choice(home, 24, replace=False), extra]))
    return np.concatenate([sk, new]), np.concatenate([lens, np.full(20, 64, np.uint32)]), J_N_OLD


C_N_OLD, C_N = 124, 130
C_ALONE = 9_000_000  # + row: a hash held by one new row alone


@functools.lru_cache(maxsize=None)
def scenario_columns():
    """130 rows at s = 64, the last 6 new.  Old rows 2 x and 2 x + 1 share 10
    hashes (62 x 10 = 620 columns among old rows only, more than a chunk) and
    each old row holds 8 hashes of its own.
      new 124: 5 of old row 3's own hashes and 5 of old row 77's -- columns
               held by exactly one new and one old row;
      new 125: the 10 hashes old rows 10 and 11 share (one new, two old);
      new 126, 127: 7 hashes the two of them share and no other row holds;
      new 128: 4 of old row 40's own and 4 of old row 120's, and 3 of the
               hashes old rows 10 and 11 share (with 125: two new, two old);
      new 129: empty.
    Every new row but 129 also holds hashes no other row holds.
    -> (sk, lens, n_old)"""
    shared = lambda x: [1_000_000 + 16 * x + e for e in range(10)]  # noqa: E731
    own = lambda g: [5_000_000 + 16 * g + e for e in range(8)]       # noqa: E731
    sets = [set(shared(g // 2)) | set(own(g)) for g in range(C_N_OLD)]
    both = [7_000_000 + e for e in range(7)]
    sets.append(set(own(3)[:5]) | set(own(77)[:5]))
    sets.append(set(shared(5)))
    sets.append(set(both))
    sets.append(set(both))
    sets.append(set(own(40)[:4]) | set(own(120)[:4]) | set(shared(5)[:3]))
    for g in range(C_N_OLD, C_N - 1):
        sets[g] |= {C_ALONE + 8 * g + e for e in range(1 + g % 3)}
    sets.append(set())
    sk = np.zeros((C_N, 64), np.uint64)
    lens = np.zeros(C_N, np.uint32)
    for g, h in enumerate(sets):
        v = np.array(sorted(h), dtype=np.uint64)
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens, C_N_OLD
