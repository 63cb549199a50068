"""The numpy model of the border schedule (tests/border_cases.py) against the
host merge, and what the scenarios of test_pairs_border_matrix_gpu.py must
contain.  No GPU."""
import pytest

import border_cases as bc
import galah_amd as ga


def host_common(sk, lens, n_old):
    """{(i, j): common} of every border pair at min_ani 0 by the host merge."""
    p = ga.pairs_border_host(sk, lens, n_old, 0.0, 21)
    return {(int(i), int(j)): int(c) for i, j, c in zip(p["i"], p["j"], p["common"])}


@pytest.mark.parametrize("n,n_old", ((1, 0), (2, 0), (2, 1), (64, 0), (65, 1), (130, 66), (130, 129), (200, 100),
                                     (193, 193), (193, 0)))
def test_numbering_and_positions(n, n_old):
    rows = bc.border_rows(n, n_old)
    assert sorted(rows) == list(range(n)) and all((r >= n_old) == (a < n - n_old) for a, r in enumerate(rows))
    order = bc.border_tile_pairs(n, n_old)
    t, tn = -(-n // 64), -(-(n - n_old) // 64)
    assert len(set(order)) == len(order) == tn * (tn + 1) // 2 + tn * (t - tn)
    assert set(order) == {(ti, tj) for ti in range(tn) for tj in range(ti, t)}
    if (n, n_old) == (200, 100):  # Tn = 2, T = 4: 3 + 4 tile pairs, the seam after the third
        assert order == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (1, 3)]


@pytest.mark.parametrize("which", ("jumps", "columns"))
def test_model_equals_the_merge(which):
    sk, lens, n_old = bc.scenario_jumps() if which == "jumps" else bc.scenario_columns()
    s = bc.BorderSchedule(sk, lens, n_old)
    ref = host_common(sk, lens, n_old)
    assert len(ref) == s.n_new * n_old + s.n_new * (s.n_new - 1) // 2  # every border pair passes at 0.0
    assert s.common() == ref  # no visited cell loses a count to a dropped column or a skipped chunk
    assert (s.n_columns, s.column_entries) == bc.dict_border_columns(sk, lens, n_old)
    exact = bc.exact_index_reads(sk, lens, n_old)
    bound = bc.index_reads_bound(s.n_columns, s.column_entries, s.new_entries)
    assert 0 < bound <= exact
    print(which, "columns", s.n_columns, "entries", s.column_entries, "new", s.new_entries, "old-only",
          s.old_only_columns, "index reads", exact, "bound", bound)


def test_jumps_scenario_contents():
    sk, lens, n_old = bc.scenario_jumps()
    s = bc.BorderSchedule(sk, lens, n_old)
    assert (s.n, s.n_new, s.tiles_new) == (300, 20, 1) and s.order == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]
    assert s.n_columns > bc.CHUNK  # more than one chunk, so that a tile can lie wholly behind the first
    # an old tile whose pieces are all empty: its tile pair ends without running a chunk
    assert s.ends_without_a_chunk() == [(0, 2)]
    # one that jumps and then runs: tile 4 holds nothing below 512
    assert (0, 4) in s.jumps_then_runs() and s.pairs[(0, 4)].events[0] == ("jump", 0, 512)
    # the mixed new / old tile row: cells with pa >= n_new that the visited rule skips
    assert s.mixed_row() == s.order and s.n_new % 64 != 0
    # chunk 0 and chunk 512 both run against tile 0 itself and against tile 1 or 3
    assert s.pairs[(0, 0)].kinds() == "rr"
    assert s.pairs[(0, 1)].runs and s.pairs[(0, 3)].runs
    # old rows unrelated to every new row have empty pieces although they share hashes among themselves
    assert all(len(s.pieces[20 + r]) == 0 for r in range(108, 172)) and s.old_only_columns > bc.CHUNK


def test_columns_scenario_contents():
    sk, lens, n_old = bc.scenario_columns()
    s = bc.BorderSchedule(sk, lens, n_old)
    assert (s.n, s.n_new) == (130, 6) and s.order == [(0, 0), (0, 1), (0, 2)]
    assert s.old_only_columns > bc.CHUNK >= s.n_columns  # the old-only columns exceed a chunk, the border's do not
    held = {}
    for r in range(s.n):
        for h in sk[r, :lens[r]].tolist():
            held.setdefault(h, []).append(r)
    kinds = {(sum(r >= n_old for r in rows), sum(r < n_old for r in rows)) for rows in held.values()}
    # (new holders, old holders): one new and one old; two new only; one new alone; one new and two old; two new and two old
    assert {(1, 1), (2, 0), (1, 0), (1, 2), (2, 2), (0, 2), (0, 1)} <= kinds
    assert s.n_columns == 10 + 10 + 7 + 8 and s.column_entries == 2 * 10 + (3 * 7 + 4 * 3) + 2 * 7 + 2 * 8
    assert s.new_entries == 10 + 10 + 14 + 11
    assert len(s.pieces[s.rows.index(129)]) == 0 and lens[129] == 0
    # old rows that no new row touches keep no id: their 620 shared hashes are no columns
    assert sum(1 for a in range(s.n_new, s.n) if len(s.pieces[a]) == 0) == 124 - 6
