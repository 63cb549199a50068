"""Inputs of the matrix-product tests that make the chunk loop jump, and a
numpy model of that loop (galah_amd/csrc/matrix_core.hpp; the kernel is
mx_common_kernel of ani_matrix.hip).  Used by test_matrix_schedule.py on the
CPU, which keeps the model honest against the host merge and pins what every
scenario must contain, and by test_matrix_jumps_gpu.py on the GPU.

The model restates the column rule and, per tile pair ti <= tj, the loop

    every row: cur = cursor_at(piece, cur, cnt, k0)    (searched from the last cursor)
    kc = next_chunk(min of tile ti's next ids, min of tile tj's)
    kc == kNoColumn: end;  kc != k0: jump (k0 = kc);  else run the chunk, k0 += 512

and records the events, the cursors of every round and the common counts of
every chunk that was run, so that a test can say which cells collect counts
after a jump and on both sides of one.
"""
import functools

import numpy as np

TILE = 64            # matrix::kTile
CHUNK = 512          # matrix::kChunk
NO_COLUMN = 0xFFFFFFFF


# ---- inputs --------------------------------------------------------------------------
def cluster_pool(c, s):
    return np.uint64(1 + (c << 20)) + np.arange(3 * s // 2, dtype=np.uint64)


def banded_clusters(n_clusters, per, s, seed, bridges=()):
    """n_clusters * per rows of s hashes, cluster c drawing from the pool
    1 + (c << 20) + arange(3 s / 2): rows in cluster order hold one contiguous
    band of column ids per cluster.  A bridge (row, cluster, cnt) replaces the
    row's cnt largest hashes by the cnt smallest of that cluster's pool, which
    gives non-zero counts between distant tiles -> (sk, lens)."""
    rng = np.random.default_rng(seed)
    n = n_clusters * per
    sk = np.zeros((n, s), np.uint64)
    for c in range(n_clusters):
        pool = cluster_pool(c, s)
        for r in range(per):
            sk[c * per + r] = np.sort(rng.choice(pool, s, replace=False))
    lens = np.full(n, s, np.uint32)
    for row, c, cnt in bridges:
        v = np.unique(np.concatenate([sk[row, :s - cnt], cluster_pool(c, s)[:cnt]]))
        sk[row] = 0
        sk[row, :len(v)] = v
        lens[row] = len(v)
    return sk, lens


def column_hash(c):
    """The hash of column c of a hand-built layout: ascending with c."""
    return 1000 + 7 * c


def rows_from_columns(holders, s, m=None):
    """holders[c] = the positions that hold column c -> (sk, lens) of m rows
    (position a is row a).  The hash ascends with c, so column c has the id c
    as long as every c has two holders or more."""
    m = 1 + max(a for h in holders for a in h) if m is None else m
    held = [[] for _ in range(m)]
    for c, h in enumerate(holders):
        assert len(set(h)) == len(h)
        for a in h:
            held[a].append(column_hash(c))
    sk = np.zeros((m, s), np.uint64)
    lens = np.zeros(m, np.uint32)
    for a, v in enumerate(held):
        assert len(v) <= s, (a, len(v))
        sk[a, :len(v)] = np.array(v, np.uint64)
        lens[a] = len(v)
    return sk, lens


# ---- the model --------------------------------------------------------------------------
def columns(sk, lens, rows):
    """The column rule over the listed positions -> (pieces, n_columns,
    column_entries): pieces[a] the ascending column ids of position a."""
    rows = [int(r) for r in rows]
    held = [sk[r, :lens[r]] for r in rows]
    if not rows or not sum(len(h) for h in held):
        return [np.zeros(0, np.int64) for _ in rows], 0, 0
    u, inv, cnt = np.unique(np.concatenate(held), return_inverse=True, return_counts=True)
    keep = cnt >= 2
    ids = np.cumsum(keep) - 1
    pieces, at = [], 0
    for h in held:
        i = inv[at:at + len(h)]
        at += len(h)
        pieces.append(ids[i[keep[i]]].astype(np.int64))
    return pieces, int(keep.sum()), int(cnt[keep].sum())


def cursor_at(piece, lo, k0):
    """matrix::cursor_at: the first index >= lo whose id is >= k0."""
    return lo + int(np.searchsorted(piece[lo:], k0, side="left"))


def next_chunk(min_a, min_b):
    if min_a == NO_COLUMN or min_b == NO_COLUMN:
        return NO_COLUMN
    return max(min_a, min_b) // CHUNK * CHUNK


class TilePair:
    """One workgroup's loop.  events: ("jump", from, to) / ("run", k0);
    rounds: (k0, lo, cur) of every search, lo / cur the cursors of the tile
    pair's positions before and after it (tile ti's positions first); runs:
    (k0, common [positions of ti x positions of tj]) of every chunk run; end:
    (k0, ids left in tile ti, ids left in tile tj) when the loop ends, counted
    as distinct ids >= k0."""

    def __init__(self, pieces, m, ti, tj):
        self.ti, self.tj, self.diag = ti, tj, ti == tj
        self.a = list(range(ti * TILE, min(m, ti * TILE + TILE)))
        self.b = list(range(tj * TILE, min(m, tj * TILE + TILE)))
        self.positions = self.a if self.diag else self.a + self.b
        self.pieces = [pieces[p] for p in self.positions]
        self.events, self.rounds, self.runs = [], [], []
        cur = [0] * len(self.positions)
        k0 = 0
        while True:
            lo = list(cur)
            cur = [cursor_at(pieces[p], c, k0) for p, c in zip(self.positions, cur)]
            self.rounds.append((k0, lo, list(cur)))
            nxt = [int(pieces[p][c]) if c < len(pieces[p]) else NO_COLUMN for p, c in zip(self.positions, cur)]
            min_a = min(nxt[:len(self.a)])
            min_b = min_a if self.diag else min(nxt[len(self.a):])
            kc = next_chunk(min_a, min_b)
            if kc == NO_COLUMN:
                break
            if kc != k0:
                self.events.append(("jump", k0, kc))
                k0 = kc
                continue
            image = np.zeros((len(self.positions), CHUNK), np.int64)
            for r, (p, c) in enumerate(zip(self.positions, cur)):
                col = pieces[p][c:] - k0  # from the cursor on, as the kernel's scatter
                image[r, col[col < CHUNK]] = 1
            ia = image[:len(self.a)]
            ib = ia if self.diag else image[len(self.a):]
            self.runs.append((k0, ia @ ib.T))
            self.events.append(("run", k0))
            k0 += CHUNK
        left = [len(np.unique(np.concatenate([pieces[p][c:] for p, c in zip(ps, cs)]))) if ps else 0
                for ps, cs in ((self.a, cur[:len(self.a)]), (self.b, cur[-len(self.b):]))]
        self.end = (k0, left[0], left[1])

    @property
    def common(self):
        """[positions of ti x positions of tj] from the chunks that were run only."""
        out = np.zeros((len(self.a), len(self.b)), np.int64)
        for _, c in self.runs:
            out += c
        return out

    def kinds(self):
        return "".join(e[0][0] for e in self.events)  # e.g. "jrjr"

    def jumps(self):
        return [e for e in self.events if e[0] == "jump"]

    def landings(self):
        """What the searches that follow a jump found, from a cursor that had
        moved before: -> {(what, k0)}, what being "k0" (a cursor at an id equal
        to k0), "k0-1" (the search passed an id equal to k0 - 1) or "k0+511" (a
        cursor at the chunk's last id)."""
        out = set()
        for n, e in enumerate(self.events):
            if e[0] != "jump":
                continue
            k0, lo, cur = self.rounds[n + 1]  # (event n is the outcome of round n)
            assert k0 == e[2]
            for pc, l, c in zip(self.pieces, lo, cur):
                if l == 0:
                    continue
                if c < len(pc) and pc[c] == k0:
                    out.add(("k0", k0))
                if c < len(pc) and pc[c] == k0 + CHUNK - 1:
                    out.add(("k0+511", k0))
                if c > l and pc[c - 1] == k0 - 1:
                    out.add(("k0-1", k0))
        return out


class Schedule:
    """chunk_schedule's result: pieces, n_columns, column_entries and
    pairs[(ti, tj)] a TilePair for every ti <= tj."""

    def __init__(self, sk, lens, rows):
        self.rows = [int(r) for r in rows]
        self.m = len(self.rows)
        self.lens = [int(lens[r]) for r in self.rows]
        self.pieces, self.n_columns, self.column_entries = columns(sk, lens, self.rows)
        self.tiles = -(-self.m // TILE)
        self.pairs = {}
        if self.m >= 2:  # (a single position has no product workgroup)
            for tj in range(self.tiles):
                for ti in range(tj + 1):
                    self.pairs[(ti, tj)] = TilePair(self.pieces, self.m, ti, tj)

    def events(self):
        return {k: p.events for k, p in self.pairs.items()}

    def n_jumps(self):
        return sum(len(p.jumps()) for p in self.pairs.values())

    def common(self):
        """The [m x m] common of every cell: the product's counts of the run
        chunks, under the diagonal rule and the empty-row rule of cell_counts."""
        m = self.m
        out = np.zeros((m, m), np.int64)
        for (ti, tj), p in self.pairs.items():
            c = p.common
            out[ti * TILE:ti * TILE + c.shape[0], tj * TILE:tj * TILE + c.shape[1]] = c
            out[tj * TILE:tj * TILE + c.shape[1], ti * TILE:ti * TILE + c.shape[0]] = c.T
        rows, lens = np.array(self.rows), np.array(self.lens)
        same = rows[:, None] == rows[None, :]
        out[same] = np.broadcast_to(lens[:, None], (m, m))[same]
        out[lens == 0, :] = 0
        out[:, lens == 0] = 0
        return out

    # ---- what a scenario must contain (each returns the tile pairs, or cells, that show it) ----
    def first_jump_then_shared(self):
        """Off-diagonal tile pairs whose first event is a jump from 0 and
        which still find a shared column: -> [((ti, tj), (a, b))], (a, b) a
        position pair whose common > 0 comes only from chunks after a jump."""
        out = []
        for k, p in self.pairs.items():
            if not p.diag and p.events and p.events[0][:2] == ("jump", 0) and p.common.any():
                r, c = np.argwhere(p.common > 0)[0]
                out.append((k, (p.a[r], p.b[c])))
        return out

    def run_jump_run(self, min_chunks=1):
        """Tile pairs with a run, a jump over min_chunks chunks or more and a
        run, and a cell that collects common on both sides of that jump."""
        out = []
        for k, p in self.pairs.items():
            for n, e in enumerate(p.events):
                if e[0] != "jump" or e[2] - e[1] < min_chunks * CHUNK:
                    continue
                before = sum((c for k0, c in p.runs if k0 < e[1]), np.zeros_like(p.common))
                after = sum((c for k0, c in p.runs if k0 >= e[2]), np.zeros_like(p.common))
                both = [(p.a[r], p.b[c]) for r, c in np.argwhere((before > 0) & (after > 0))
                        if self.rows[p.a[r]] != self.rows[p.b[c]]]  # (the same row: the diagonal rule, no product)
                if both:
                    out.append((k, both[0]))
                    break
        return out

    def run_jump_run_events(self):
        """Tile pairs whose events hold a run, later a jump, later a run."""
        out = []
        for k, p in self.pairs.items():
            kinds = p.kinds()
            if any("r" in kinds[:n] and "r" in kinds[n + 1:] for n, x in enumerate(kinds) if x == "j"):
                out.append(k)
        return out

    def jump_without_run(self):
        return [k for k, p in self.pairs.items() if not p.diag and p.jumps() and not p.runs]

    def diagonal_with_jump(self):
        return [k for k, p in self.pairs.items() if p.diag and p.jumps()]

    def ends_with_ids_left(self, at_least=CHUNK):
        """Tile pairs that end because one tile is exhausted while the other
        still holds at_least ids."""
        return [k for k, p in self.pairs.items()
                if not p.diag and min(p.end[1:]) == 0 and max(p.end[1:]) >= at_least]

    def last_tile_not_full(self):
        return self.m % TILE != 0


def chunk_schedule(sk, lens, rows=None):
    return Schedule(sk, lens, range(len(lens)) if rows is None else rows)


def group_schedules(sk, lens, groups):
    """chunk_schedule per group: the grouped column rule sees one group's
    positions only, and a group's ids begin at 0."""
    return [Schedule(sk, lens, g) for g in groups]


def dict_columns(sk, lens, rows):
    """(columns, column entries) of the listed positions from a dict, without the model."""
    held = {}
    for r in rows:
        for h in sk[r, :lens[r]].tolist():
            held[h] = held.get(h, 0) + 1
    return sum(1 for c in held.values() if c >= 2), sum(c for c in held.values() if c >= 2)


# ---- the scenarios ------------------------------------------------------------------------
A_BRIDGES = ((3, 29, 20), (298, 0, 20), (70, 15, 10))


@functools.lru_cache(maxsize=None)
def scenario_a():
    """30 clusters of 10 rows at s = 64 in cluster order, three bridged rows:
    300 rows, 5 tiles, the last of 44 -> (sk, lens)."""
    return banded_clusters(30, 10, 64, seed=1, bridges=A_BRIDGES)


A_TWICE = (5, 200)  # scenario A's row 5 is listed again at position 200: tiles 0 and 3


def scenario_a_listed():
    """Scenario A's rows through a row list, one row at two positions of different tiles."""
    rows = list(range(300))
    rows[A_TWICE[1]] = A_TWICE[0]
    return rows


B_COLUMNS = 2560
B_S = 128


@functools.lru_cache(maxsize=None)
def scenario_b():
    """Boundary ids after a jump, hand-built: 2,560 columns, every one held by
    two rows of tile 3 (the filler: column c at positions 192 + c % 64 and
    192 + (c + 32) % 64), so that column c has the id c.

      tile 0 (positions 0 .. 63): position r holds the 72 ids 8 r .. 8 r + 71
        modulo 512 (together 0 .. 511; more than the 64 entries one step of
        the kernel's scatter takes, so a cursor kept from before a jump loses
        what follows), then nothing until 1535 (positions 0 .. 31); then
        2048 + r (positions 0 .. 15), 2559 (positions 16 .. 47) or nothing.
      tile 1 (positions 64 .. 127) starts at 1023; by position modulo 8:
        0: 1023 1024 1535 1536 2047 2048      1: 1024 1536 2048
        2: 1023 1535 2047                     3: 1023 1536 2047 2559
        4: 1024 1535 2048                     5: 1535 2559
        6: 2047                               7: 1536 2048 2049
      tile 2 (positions 128 .. 191): tile 1's ids, and the id r before them.

    Tile pair (0, 1) jumps 0 -> 512 -> 1024, runs 1024, jumps 1536 -> 2048,
    runs 2048.  Tile pair (0, 2) runs 0, jumps 512 -> 1024 with tile 2's
    cursors at 1 already, runs 1024, jumps to 2048, runs 2048.
    -> (sk, lens) of 256 rows at s = 128."""
    tile1 = ((1023, 1024, 1535, 1536, 2047, 2048), (1024, 1536, 2048), (1023, 1535, 2047), (1023, 1536, 2047, 2559),
             (1024, 1535, 2048), (1535, 2559), (2047,), (1536, 2048, 2049))
    holders = [[192 + c % 64, 192 + (c + 32) % 64] for c in range(B_COLUMNS)]
    for r in range(64):
        ids = sorted((8 * r + j) % 512 for j in range(72))
        if r < 32:
            ids.append(1535)
        if r < 16:
            ids.append(2048 + r)
        elif r < 48:
            ids.append(2559)
        for c in ids:
            holders[c].append(r)
        for c in tile1[r % 8]:
            holders[c].append(64 + r)
            holders[c].append(128 + r)
        holders[r].append(128 + r)
    return rows_from_columns(holders, B_S, 256)


C_FIRST_OFFSET = np.uint64(1 << 40)


@functools.lru_cache(maxsize=None)
def scenario_c():
    """The grouped form -> (sk, lens, groups) at s = 64.
      group 0: 28 rows (14 banded clusters of 2, hashes of their own) with
        more than 512 columns, so that the ids of every later group are large
        before they are made local;
      group 1: scenario A's 300 rows;
      group 2: one row (of scenario A: a row may be listed in several groups);
      group 3: 100 rows (2 tiles) drawn anew from the pools of scenario A's
        clusters 0 .. 9, so that the same hash is a column in two groups."""
    a_sk, a_lens = scenario_a()
    f_sk, f_lens = banded_clusters(14, 2, 64, seed=5)
    f_sk = f_sk + C_FIRST_OFFSET
    d_sk, d_lens = banded_clusters(10, 10, 64, seed=3, bridges=((2, 9, 20), (97, 0, 20)))
    sk = np.concatenate([a_sk, f_sk, d_sk])
    lens = np.concatenate([a_lens, f_lens, d_lens])
    groups = [list(range(300, 328)), list(range(300)), [7], list(range(328, 428))]
    return sk, lens, groups


D_BRIDGES = ((3, 39, 20), (198, 0, 20), (70, 20, 10))


@functools.lru_cache(maxsize=None)
def scenario_d():
    """40 clusters of 5 rows at s = 128, listed in a fixed permuted order: a
    tile holds rows of many clusters, but not of all -> (sk, lens, rows)."""
    sk, lens = banded_clusters(40, 5, 128, seed=1, bridges=D_BRIDGES)
    rows = [int(r) for r in np.random.default_rng(2).permutation(200)]
    return sk, lens, rows


# ---- the small edges of the prologue ---------------------------------------------------------
H_MAX = 2 ** 64 - 1


@functools.lru_cache(maxsize=None)
def extreme_hash_rows():
    """Hashes 0 and 2^64 - 1 as columns, every row shorter than s = 64 (the
    sort's padding is the key ~0, a row's unused slots hold 0):
      rows 0 and 1 share 0 and 10; row 2 ends in 2^64 - 1 and holds nothing
      else that is a column; row 3 holds it too; row 4 holds it alone; row 5
      is empty; row 6 holds 0 alone; row 7 shares 20 and 30 with rows 0 and 3.
    -> (sk, lens)"""
    sets = [{0, 10, 20, 30}, {0, 10, 40}, {7, 8, 9, H_MAX}, {20, 30, 50, H_MAX}, {H_MAX}, set(), {0}, {20, 30, 60, 61}]
    sk = np.zeros((len(sets), 64), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for g, h in enumerate(sets):
        v = np.array(sorted(h), dtype=np.uint64)
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens


EXTREME_GROUPS = (
    [[0, 1, 2, 3], [4, 5, 6, 0]],       # rows 2 and 3 in one group: 2^64 - 1 is a column there, and in no other
    [[0, 1, 2, 6], [3, 7, 5], [4, 1]],  # its three holders in three groups: a column of none
)


OFFSETS_MIN_ANI = 0.99  # passes the fuller rows of a cluster, not the short ones


@functools.lru_cache(maxsize=None)
def offsets_rows():
    """2,100 rows at s = 16 in clusters of 3 that draw from a pool of 18
    hashes, lengths mixed from 0 to 16: mx_offsets_kernel gives 32 positions to
    a thread, so 66 threads hold positions and the scan of their sums crosses
    the first wave -> (sk, lens)."""
    rng = np.random.default_rng(2100)
    m, s = 2100, 16
    sk = np.zeros((m, s), np.uint64)
    lens = rng.integers(0, s + 1, m).astype(np.uint32)
    lens[rng.random(m) < 0.5] = s
    for c in range(m // 3):
        pool = np.uint64(1 + c * 64) + np.arange(18, dtype=np.uint64)
        for r in range(3 * c, 3 * c + 3):
            sk[r, :lens[r]] = np.sort(rng.choice(pool, int(lens[r]), replace=False))
    return sk, lens
