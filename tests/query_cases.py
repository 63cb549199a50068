"""Scenarios of the query tests (tests/test_query.py on the host forms,
tests/test_query_gpu.py on the device): each a function returning (rows, lens,
q_rows, q_lens), with asserts on what it must contain, and the reference every
form is held to: the CPU oracle's pairs of rows ++ queries, filtered to
i < n <= j."""
import functools

import numpy as np

import oracle
from test_pair_edges import max_sketch_rows, quads, sweep_reference, sweep_rows

f32 = np.float32
U64_MAX = np.uint64(2**64 - 1)
WAVES_PER_WORKGROUP = 4  # query.hip kQueryWaves


def matrix(sets, s):
    """Sorted hash sets -> ([len(sets), s] u64 zero-padded, lens u32)."""
    sk = np.zeros((len(sets), s), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for i, v in enumerate(sets):
        v = np.unique(np.asarray(v, dtype=np.uint64))
        assert len(v) <= s
        sk[i, :len(v)] = v
        lens[i] = len(v)
    return sk, lens


def shared_hashes(case):
    """The distinct hashes that some row and some query both hold."""
    rows, lens, q_rows, q_lens = case
    a = np.concatenate([rows[i, :lens[i]] for i in range(len(lens))] + [np.zeros(0, np.uint64)])
    b = np.concatenate([q_rows[i, :q_lens[i]] for i in range(len(q_lens))] + [np.zeros(0, np.uint64)])
    return np.intersect1d(a, b)


def columns(case):
    """The distinct hashes of the queries: the columns of a table over all of them."""
    _, _, q_rows, q_lens = case
    return len(np.unique(np.concatenate([q_rows[i, :q_lens[i]] for i in range(len(q_lens))] + [np.zeros(0, np.uint64)])))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- sweep ---------------------------------------------------------------------
SWEEP_SPLITS = (536, 599, 1, 300)


def sweep(n):
    """test_pair_edges.sweep_rows() split n | 600 - n: ~1,000 distinct (common,
    total), equal last elements, every lens."""
    sk, lens = sweep_rows()
    assert 0 < n < len(lens) and set(lens.tolist()) == set(range(1, sk.shape[1] + 1))
    return sk[:n], lens[:n], sk[n:], lens[n:]


def sweep_expected(n, thr, k):
    """[m, 4] in (i, j) order and the f64 ANI of the cells of sweep(n) that pass at thr."""
    q, ani, _ = sweep_reference(k)
    keep = (ani >= np.float64(thr)) & (q[:, 0] < n) & (q[:, 1] >= n)
    return q[keep], ani[keep]


# ---- table -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    """s = 64: what the slot function, the empty mark and the columns must survive."""
    rng = np.random.default_rng(64)
    s = 64
    base = np.unique(rng.integers(1, 2**44, 4 * s, dtype=np.uint64))  # real-sketch-like: high bits zero
    low = (np.arange(1, 301, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xDEADBEEF)  # equal low 32 bits
    high = (np.uint64(0xABCDEF01) << np.uint64(32)) | np.arange(1, 301, dtype=np.uint64)  # equal high 32 bits
    pool = np.concatenate([low, high])
    ends = [np.uint64(0), U64_MAX]
    pool = rng.permutation(pool)
    spread = [np.sort(pool[t * s:(t + 1) * s]) for t in range(5)]  # 320 of the 600
    dup = base[10:74]
    queries = [
        np.concatenate([ends, base[:62]]),  # 0: holds 0 and 2^64 - 1
        spread[0], spread[1],
        dup,                                # 3: one query three times
        np.zeros(0, np.uint64),             # 4: an empty query between non-empty ones
        dup, spread[2], dup, spread[3], spread[4],
    ]
    rows = [
        np.concatenate([ends, base[:62]]),        # 0: query 0 itself
        np.concatenate([ends, base[1:63]]),       # 1
        np.array(ends, np.uint64),                # 2: 0 and 2^64 - 1 alone
        dup,                                      # 3: equal to a query: ANI 1.0
        np.zeros(0, np.uint64),                   # 4: an empty row
    ]
    for r in range(8):  # a spread query with 35 entries swapped for the other 280 of the pool (ANI ~0.96)
        v = spread[r % 5].copy()
        v[rng.choice(s, 35, replace=False)] = pool[320 + r * 35:320 + (r + 1) * 35]
        rows.append(v)
    case = matrix(rows, s) + matrix(queries, s)
    sk, lens, q_sk, q_lens = case
    both = shared_hashes(case)
    assert np.uint64(0) in both and U64_MAX in both
    assert sum(int(x in (0, 2**64 - 1)) for r in range(3) for x in sk[r, :lens[r]].tolist()) == 6
    used = np.unique(np.concatenate([sk[5:].ravel(), q_sk[[1, 2, 6, 8, 9]].ravel()]))
    assert np.isin(low, used).all() and np.isin(high, used).all()
    assert (q_sk[3] == q_sk[5]).all() and (q_sk[3] == q_sk[7]).all() and (sk[3] == q_sk[3]).all() and lens[3] == s
    assert q_lens[4] == 0 and q_lens[3] and q_lens[5] and lens[4] == 0
    return frozen(*case)


@functools.lru_cache(maxsize=None)
def empty_queries():
    """A batch whose queries are all empty: nothing is built, nothing found."""
    sk, lens, _, _ = table()
    q_sk, q_lens = np.zeros((3, 64), np.uint64), np.zeros(3, np.uint32)
    return frozen(sk, lens, q_sk, q_lens)


@functools.lru_cache(maxsize=None)
def column_count(c):
    """One query of c hashes (32: the smallest table is exactly half full; 33:
    the next capacity), rows that hold all, some and none of them."""
    rng = np.random.default_rng(c)
    s = 64
    v = np.unique(rng.integers(1, 2**44, 2 * s, dtype=np.uint64))
    case = matrix([v[:c], v[:c - 1], v[1:c + 3], v[c + 5:c + 40], v[:c][::2]], s) + matrix([v[:c]], s)
    assert columns(case) == c and case[1][0] == c
    return frozen(*case)


# ---- sparse ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse():
    """4,999 rows at s = 64 that hold no hash of any query, except rows 0,
    2,500 and 4,998 and five clusters of 6 that three queries belong to."""
    rng = np.random.default_rng(4999)
    n, s = 4999, 64
    assert n % WAVES_PER_WORKGROUP != 0
    sk = np.sort(rng.integers(1, 2**62, (n, s), dtype=np.uint64), axis=1)
    centres = np.sort(rng.integers(2**62, 2**63, (8, s + 8), dtype=np.uint64), axis=1)

    def member(c):
        v = np.unique(centres[c])
        return np.sort(rng.choice(v, s, replace=False))  # 64 of the centre's 72: ANI to another member ~0.99

    cluster_rows = {}
    for c in range(5):
        for x in range(6):
            r = 100 + c * 977 + x * 13
            sk[r] = member(c)
            cluster_rows.setdefault(c, []).append(r)
    for r, c in ((0, 5), (2500, 6), (4998, 7)):
        sk[r] = member(c)
    queries = [member(0), member(2), member(4), member(5), member(6), member(7),
               np.sort(rng.integers(2**63, 2**64 - 1, s, dtype=np.uint64))]  # the last: unrelated to every row
    lens = np.full(n, s, np.uint32)
    case = (sk, lens) + matrix(queries, s)
    assert (sk[:, 1:] > sk[:, :-1]).all()
    hit = np.isin(sk, np.concatenate([q for q in queries[:6]])).any(axis=1)
    expect = {0, 2500, 4998} | {r for c in (0, 2, 4) for r in cluster_rows[c]}
    assert set(np.nonzero(hit)[0].tolist()) == expect and len(expect) == 21
    return frozen(*case)


# ---- large s, small s ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_s():
    """24 adversarial rows at s = 12,000 with identical rows, split 20 | 4: the counters reach 12,000."""
    sk, lens = max_sketch_rows()
    assert any((sk[i] == sk[20]).all() and lens[i] == 12000 for i in range(20))
    return sk[:20], lens[:20], sk[20:], lens[20:]


@functools.lru_cache(maxsize=None)
def one_hash():
    return frozen(*(matrix([[5], [7], [5], [], [9]], 1) + matrix([[5], [], [9], [11]], 1)))


@functools.lru_cache(maxsize=None)
def lens_around_64():
    """s = 65 with lens 63, 64 and 65 on both sides: a lane's second hash, or none."""
    rng = np.random.default_rng(65)
    v = np.unique(rng.integers(1, 2**50, 200, dtype=np.uint64))
    rows = [v[:63], v[:64], v[:65], v[1:66], v[2:65], v[100:163]]
    queries = [v[:65], v[:64], v[:63], v[3:68]]
    case = matrix(rows, 65) + matrix(queries, 65)
    assert sorted(set(case[1].tolist())) == [63, 64, 65] and sorted(set(case[3].tolist())) == [63, 64, 65]
    return frozen(*case)


# name -> (scenario, sketch size); the sweep has tests of its own thresholds
CASES = {
    "sweep_536": (lambda: sweep(536), 32), "sweep_599": (lambda: sweep(599), 32), "sweep_1": (lambda: sweep(1), 32),
    "sweep_300": (lambda: sweep(300), 32),
    "table": (table, 64), "empty_queries": (empty_queries, 64), "columns_32": (lambda: column_count(32), 64),
    "columns_33": (lambda: column_count(33), 64), "sparse": (sparse, 64), "large_s": (large_s, 12000),
    "one_hash": (one_hash, 1), "lens_around_64": (lens_around_64, 65),
}
ORACLE_ROWS = 1500  # more rows than this: the oracle runs on the rows that share a hash with a query


@functools.lru_cache(maxsize=None)
def expected(name, thr_bits, k=21):
    """[m, 4] (i, n + q, common, total) in (i, j) order of scenario `name` at
    the f32 threshold with bits thr_bits, from the oracle."""
    thr = np.uint32(thr_bits).view(f32)
    sk, lens, q_sk, q_lens = CASES[name][0]()
    n = len(lens)
    if name.startswith("sweep_"):
        return sweep_expected(n, thr, k)[0]
    rows = np.arange(n)
    if n > ORACLE_ROWS:
        # a row without a shared hash has common 0 with every query: ANI exactly 0, below any thr > 0
        assert thr > 0
        valid = np.arange(sk.shape[1])[None, :] < lens[:, None]
        q_valid = np.arange(q_sk.shape[1])[None, :] < q_lens[:, None]
        rows = np.nonzero((np.isin(sk, q_sk[q_valid]) & valid).any(axis=1))[0]
    m = len(rows)
    all_sk = np.concatenate([sk[rows], q_sk])
    all_lens = np.concatenate([lens[rows], q_lens]).astype(np.int32)
    q = quads(oracle.pairs(all_sk, all_lens, thr, k=k))
    q = q[(q[:, 0] < m) & (q[:, 1] >= m)]
    q[:, 1] += np.uint32(n - m)
    q[:, 0] = rows[q[:, 0]]
    q.setflags(write=False)
    return q


def bits(thr):
    return int(f32(thr).view(np.uint32))
