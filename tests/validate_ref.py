"""Restatement of what cluster validation computes, for the tests
(test_validate.py on the CPU, test_validate_gpu.py on the GPU), in plain
Python and as literally as the reference has it:

  src/finch.rs:57 -> finch::distance::distance: the merge loop over two
      ascending sketches until either is exhausted;
  src/cluster_validation.rs:21-45, :47-77: the two loops of validate_clusters,
      finch's f32 ANI in FastANI's place.

The only library function used is ani_f32 (the stored value of a (common,
total); its arithmetic is pinned by test_host.py).  Also the synthetic sketch
rows both test files share.
"""
import numpy as np

import galah_amd as ga


def merge(a, b):
    """(common, total) of two ascending rows."""
    la, lb = len(a), len(b)
    i = j = common = 0
    while i < la and j < lb:
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
    return common, i + j - common


def merge_rows(sketches, lens, i, j):
    return merge(sketches[i][:lens[i]].tolist(), sketches[j][:lens[j]].tolist())


def ani_pairs_ref(sketches, lens, pairs, k=21):
    """[(common, total)], [f32] of the named pairs, in the order given."""
    counts = [merge_rows(sketches, lens, int(i), int(j)) for i, j in pairs]
    return counts, [ga.ani_f32(c, t, k) for c, t in counts]


def validate_ref(sketches, lens, clusters, threshold, k=21):
    """-> (member_pairs, member_bad list, rep_pairs, rep_bad list); a bad
    entry is (i, j, common, total, f32 ani), members as (rep, member) sorted
    so with one entry per listing, representatives as (r1 <= r2) sorted."""
    thr = np.float32(threshold)
    member_pairs, member_bad = 0, []
    for cluster in clusters:  # :21-45
        rep = cluster[0]
        for genome in cluster[1:]:
            if genome == rep:
                continue  # (the reference compares it with itself; the library does not)
            member_pairs += 1
            c, t = merge_rows(sketches, lens, rep, genome)
            ani = ga.ani_f32(c, t, k)
            if not ani >= thr:
                member_bad.append((rep, genome, c, t, ani))
    reps = [c[0] for c in clusters]
    rep_pairs, rep_bad = 0, []
    for i, rep1 in enumerate(reps):  # :47-77
        for j, rep2 in enumerate(reps):
            if i < j:
                rep_pairs += 1
                c, t = merge_rows(sketches, lens, rep1, rep2)
                ani = ga.ani_f32(c, t, k)
                if not ani < thr:
                    rep_bad.append((min(rep1, rep2), max(rep1, rep2), c, t, ani))
    return member_pairs, sorted(member_bad, key=lambda r: r[:2]), rep_pairs, sorted(rep_bad, key=lambda r: r[:2])


def as_tuples(v):
    """A ga.Validation in validate_ref's form."""
    rows = [(int(p["i"]), int(p["j"]), int(p["common"]), int(p["total"]), np.float32(a))
            for p, a in zip(v.bad, v.bad_ani)]
    assert len(rows) == v.member_bad + v.rep_bad
    return v.member_pairs, rows[:v.member_bad], v.rep_pairs, rows[v.member_bad:]


def error_lines(ref, genomes):
    """The reference's error! lines (:31-34, :62-65) for validate_ref's result."""
    hundred = np.float32(100)
    _, member_bad, _, rep_bad = ref
    out = ["finch ANI between %s and %s is not ok: %s" % (genomes[r], genomes[g], ga.rust_f32(a * hundred))
           for r, g, _, _, a in member_bad]
    out += ["finch ANI between reps %s and %s is not ok: %s" % (genomes[a], genomes[b], ga.rust_f32(v * hundred))
            for a, b, _, _, v in rep_bad]
    return out


def clusters_of(rep_of):
    """rep_of -> clusters, by representative ascending, representative first."""
    rep_of = [int(r) for r in rep_of]
    return [[r] + [g for g, x in enumerate(rep_of) if x == r and g != r] for r in sorted(set(rep_of))]


# ---- synthetic rows ------------------------------------------------------------
EDGE_LENS = (0, 1, 2, 63, 64, 65)


def synth_rows(s, lens, seed, shared=0.5):
    """[len(lens) x s] ascending rows without repeats whose hashes come from
    one pool of ~2 s values, so that rows share about half their hashes and
    their last elements interleave."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, 1 << 63, size=4 * s + 8, dtype=np.uint64))
    pool = pool[:max(2 * s, 2)] if shared else pool
    sk = np.zeros((len(lens), s), dtype=np.uint64)
    for g, l in enumerate(lens):
        sk[g, :l] = np.sort(rng.choice(pool, size=l, replace=False))
    return sk, np.asarray(lens, dtype=np.uint32)


def edge_case(s, seed=0):
    """Rows whose lengths are drawn from {0, 1, 2, 63, 64, 65, s} (those that
    fit s), every length at least once, and all their ordered pairs, i == j
    included."""
    lens = sorted({l for l in EDGE_LENS + (s,) if l <= s})
    lens = lens + lens[1:]  # each non-empty length twice, from different draws
    sk, ln = synth_rows(s, lens, 100 + s + seed)
    n = len(lens)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    return sk, ln, pairs


def shape_case(s=96):
    """The shapes a merge can take, by name -> (sketches, lens, pairs)."""
    base = np.arange(1, 2 * s + 1, dtype=np.uint64) * np.uint64(1000)
    rows = {
        "a": base[:s],                       # 1000 .. s * 1000
        "a_again": base[:s].copy(),          # identical to a
        "disjoint_above": base[s:2 * s],     # all of a below all of it
        "subset": base[:s:3],                # a subset of a (every third), smaller last element
        "subset_same_last": np.concatenate([base[1:s:4], base[s - 1:s]]),  # a subset sharing a's last element
        "interleaved": base[:s] + np.uint64(1),  # no common hash, values between a's
        "one": base[5:6],
        "empty": base[:0],
    }
    names = sorted(rows)
    sk = np.zeros((len(names), s), dtype=np.uint64)
    lens = np.zeros(len(names), dtype=np.uint32)
    for g, name in enumerate(names):
        r = np.unique(rows[name])
        sk[g, :len(r)] = r
        lens[g] = len(r)
    pairs = [(i, j) for i in range(len(names)) for j in range(len(names))]
    return names, sk, lens, pairs
