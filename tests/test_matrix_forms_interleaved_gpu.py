"""The four forms of the matrix product on one context, one after another
(galah_amd/csrc/ani_matrix.hip): border, grouped, dense and
pair calls share one positions part and its context scratch -- the two sort
buffers that the flags and ids alias, the border's run starts in the value and
piece buffers, the grouped form's second sort or its memset of the group
words.  Every other matrix file mostly drives one form; a stale or wrong alias
shows only when a call follows one of another form or of another size.

The sequence, twice through on the same context at sketch size 64:

  1. border, n = 130, n_old = 70 (the 60 new rows in one tile of three);
  2. groups of 1, 2, 65, 130, 0 and 1 rows (the second sort on the group bits);
  3. one group of 130 rows (the memset of the group words instead);
  4. dense, m = 193 through a shuffled row list;
  5. pairs at m = 64, then at m = 193 (the scratch in use shrinks, then grows);
  6. border with n_old = 0 and with n_old = n - 1.

The references and the equality are those of each form's own file: the host
merge (ani_matrix_host, ani_matrix_groups_host: common, total and the f32 bit
pattern equal; pairs_border_host: the sorted (i, j, common, total) tuples),
without tolerance, computed once.  The summaries of the second time through
equal those of the first."""
import numpy as np
import pytest

import galah_amd as ga
import matrix_cases as mc

pytestmark = pytest.mark.gpu

F = lambda x: float(np.float32(x))  # noqa: E731  (a threshold as the f32 the library takes)
THR = F(0.9)
BORDER_N = 130
GROUP_SIZES = (1, 2, 65, 130, 0, 1)
COUNTS = ("n_entries", "n_columns", "column_entries")


def tuples(p):
    return list(zip(p["i"].tolist(), p["j"].tolist(), p["common"].tolist(), p["total"].tolist()))


def pairs_reference(sk, lens, min_ani, rows):
    """The passing pairs of the listed rows by the host merge, sorted tuples of row indices."""
    rows = np.asarray(rows, dtype=np.int64)
    p = ga.pairs_border_host(sk[rows], lens[rows], 0, min_ani)
    a, b = rows[p["i"]], rows[p["j"]]
    return sorted(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist(), p["common"].tolist(), p["total"].tolist()))


@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def cases():
    """matrix_cases.scenario_a's 300 banded rows -> the calls of the sequence
    and their references: [(name, call(ctx) -> (result, summary), reference)]."""
    sk, lens = mc.scenario_a()
    perm = [int(r) for r in np.random.default_rng(193).permutation(300)]
    groups, at = [], 0
    for m in GROUP_SIZES:
        groups.append(perm[at:at + m])
        at += m
    one_group = [perm[100:230]]
    listed = perm[:193]
    bsk, blens = sk[:BORDER_N], lens[:BORDER_N]

    def border(n_old):
        ref = tuples(ga.pairs_border_host(bsk, blens, n_old, THR))

        def call(ctx):
            pairs, summary = ctx.pairs_border_matrix(bsk, blens, n_old, THR)
            assert summary["path"] == "matrix" and summary["n_pairs"] == len(pairs)
            return tuples(pairs), summary
        return "border n_old=%d" % n_old, call, ref

    def grouped(name, gs):
        ref = ga.ani_matrix_groups_host(sk, lens, gs)

        def call(ctx):
            common, total, ani, cells, summary = ctx.ani_matrix_groups(sk, lens, gs)
            return (common, total, ani, cells), summary
        return name, call, ref

    def dense(rows):
        ref = ga.ani_matrix_host(sk, lens, rows)

        def call(ctx):
            common, total, ani, summary = ctx.ani_matrix(sk, lens, rows)
            return (common, total, ani), summary
        return "dense m=%d" % len(rows), call, ref

    def pairs(rows):
        ref = pairs_reference(sk, lens, THR, rows)

        def call(ctx):
            p, summary = ctx.pairs_matrix(sk, lens, THR, rows)
            assert summary["path"] == "matrix" and summary["n_pairs"] == len(p)
            return tuples(p), summary
        return "pairs m=%d" % len(rows), call, ref

    seq = [border(70), grouped("groups %r" % (GROUP_SIZES,), groups), grouped("one group of 130", one_group),
           dense(listed), pairs(listed[:64]), pairs(listed), border(0), border(BORDER_N - 1)]
    # what the inputs must contain for the sequence to mean anything
    by = {name: ref for name, _, ref in seq}
    assert 0 < len(by["border n_old=70"]) < 60 * 70 + 60 * 59 // 2
    assert 0 < len(by["pairs m=64"]) < len(by["pairs m=193"]) < 193 * 192 // 2
    assert len(by["border n_old=0"]) > len(by["border n_old=70"]) > len(by["border n_old=129"]) > 0
    assert by["groups %r" % (GROUP_SIZES,)][3].tolist() == np.concatenate(
        [[0], np.cumsum([m * m for m in GROUP_SIZES])]).tolist()
    return seq


def assert_same(name, got, ref):
    if isinstance(ref, list):  # a pair list: sorted tuples
        assert sorted(got) == sorted(ref) and len(set(got)) == len(got), \
            "%s: %d pairs, the merge passes %d" % (name, len(got), len(ref))
        return
    for what, g, r in zip(("common", "total", "ani", "cells"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (name, what)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint32 if g.itemsize == 4 else np.uint64)
                              != r.view(np.uint32 if r.itemsize == 4 else np.uint64))
            at = tuple(int(x) for x in bad[0])
            raise AssertionError("%s %s: %d cells differ, first %r: %r, expected %r"
                                 % (name, what, len(bad), at, g[at], r[at]))


def test_forms_interleaved_on_one_context(ctx64, cases):
    first = {}
    for time_through in (1, 2):
        for name, call, ref in cases:
            got, summary = call(ctx64)
            assert_same("%s (time %d)" % (name, time_through), got, ref)
            counts = tuple(summary[f] for f in COUNTS)
            print("%s (time %d): %s" % (name, time_through, dict(zip(COUNTS, counts))))
            assert counts[0] > 0 and 0 < 2 * counts[1] <= counts[2] <= counts[0], name
            if time_through == 1:
                first[name] = counts
            else:
                assert counts == first[name], name
