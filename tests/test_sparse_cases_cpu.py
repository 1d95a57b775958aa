"""CPU: the inputs of tests/test_gpu_sparse_sums.py (tests/sparse_cases.py) reach the paths they are there for, at the 256 CUs of an
MI355X, and the host references agree with Python integers on every planted row."""
import numpy as np
import pytest
import pyref as P
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
import sparse_cases as SC

CU = 256
W4, W1 = SC.waves4(CU), SC.waves1(CU)


def _row_lens(r1cs, name):
    rp = np.asarray(r1cs[name][0], np.uint64).astype(np.int64)
    return rp[1:] - rp[:-1]


@pytest.mark.parametrize("heavy", "ABC")
def test_rows_past_one_grid(heavy):
    r1cs = SC.rows_past_one_grid(CU, heavy)
    assert 8900 < r1cs["n_constraints"] < 9100 and r1cs["nb_wires"] == 4096
    want = SC.rows_counts(CU)
    assert sorted(r1cs["roles"]) == sorted((RC.HEAVY, RC.ONE, RC.NONE)) and r1cs["roles"]["ABC".index(heavy)] == RC.HEAVY
    W = RC.witness(r1cs["nb_wires"], 7)
    for name, role in zip("ABC", r1cs["roles"]):
        assert RC.split_counts(r1cs, name) == want[role], f"{name} ({role})"      # the imbalance: thousands, one, zero
        lens = _row_lens(r1cs, name)
        rows, planted_lens = r1cs["planted"][name]
        assert len(set(rows.tolist())) == len(rows) == want[role][0] and np.array_equal(lens[rows], planted_lens)
        assert int((lens > RC.SHORT).sum()) == len(rows) and set(range(5)) <= set(lens.tolist())
        ref = RC.eval_rows(r1cs, name, W)
        for i in rows:
            assert S._int(ref[i]) == RC.row_by_integers(r1cs, name, W, int(i)), f"{name} row {i}"
    n_long, n_pieces = want[RC.HEAVY]
    assert n_long > W4 and n_pieces > W4 and sorted(set(r1cs["planted"][heavy][1].tolist())) == [RC.SHORT + 1, RC.CHUNK + 1]
    # every `which` that names the heavy matrix is past one grid in both wave passes; the others hold one long row at the most
    for which in range(1, 8):
        names = "".join(n for k, n in enumerate("ABC") if which & (1 << k))
        got = RC.split_counts(r1cs, names)
        assert (got[0] > W4 and got[1] > W4) if heavy in names else got[0] <= 1


@pytest.mark.parametrize("heavy", "ABC")
def test_rows_past_one_grid_made_solvable(heavy):
    src = SC.rows_past_one_grid(CU, heavy)
    r1cs, W, a, b, c = RC.with_slack(src, RC.witness(src["nb_wires"], 7))
    nc = src["n_constraints"]
    assert r1cs["nb_wires"] == src["nb_wires"] + nc == len(W) and r1cs["slack0"] == src["nb_wires"]
    assert all(RC.split_counts(r1cs, name) == RC.split_counts(src, name) for name in "ABC")       # one entry more per row of C cuts nothing anew
    assert np.array_equal(_row_lens(r1cs, "C"), _row_lens(src, "C") + 1) and r1cs["A"] is src["A"] and r1cs["B"] is src["B"]
    count = np.bincount(np.concatenate([r1cs[name][1] for name in "ABC"]), minlength=r1cs["nb_wires"])
    assert (count[r1cs["slack0"]:] == 1).all()
    ref = RC.eval_all(r1cs, W)
    for have, want in zip(ref, (a, b, c)):
        assert np.array_equal(have, want)
    assert RC.check_rows(*ref) == (0, RC.U64_MAX)
    rows = SC.pinned_rows(src, CU)
    order = np.nonzero(_row_lens(src, heavy) > RC.SHORT)[0]        # the library's list of long rows: ascending by row
    assert [int(np.searchsorted(order, r)) for r in rows[:4]] == [0, W4 - 1, W4, len(order) - 1] and all(order[np.searchsorted(order, r)] == r for r in rows[:4])
    assert len(set(rows[:4])) == 4 and len(rows) == 6 and max(_row_lens(src, n)[rows[5]] for n in "ABC") <= 4
    for i in rows:
        assert S._int(ref[2][i]) == RC.row_by_integers(r1cs, "C", W, i)
        assert RC.check_rows(*RC.eval_all(r1cs, RC.bumped(W, [r1cs["slack0"] + i]))) == (1, i)


def test_every_which_is_past_one_grid_under_some_role():
    for which in range(1, 8):
        assert any(which & (1 << "ABC".index(heavy)) for heavy in "ABC")


def test_transposed_columns_past_one_grid():
    src = SC.rows_past_one_grid(CU, "A")
    r1cs = RC.transposed(src)
    assert r1cs["n_constraints"] == 4096 and r1cs["nb_wires"] == src["n_constraints"]
    for name in "ABC":
        lens = np.bincount(r1cs[name][1], minlength=r1cs["nb_wires"])
        assert np.array_equal(lens, _row_lens(src, name)) and len(r1cs[name][1]) == len(src[name][1])
        rows, planted_lens = src["planted"][name]
        assert np.array_equal(lens[rows], planted_lens)
    assert RC.split_counts(src)[0] > W4 and RC.split_counts(src)[1] > W4
    # the transpose is the same matrix: row j of M times x against column j of the transpose in integers, on the planted lists
    x = RC.witness(r1cs["n_constraints"], 11)
    for name in "AB":
        rows_x = RC.eval_rows(src, name, x)
        for j in src["planted"][name][0][::97]:
            assert S._int(rows_x[j]) == S.column_by_integers(r1cs, name, x, int(j)), f"{name} column {j}"


def test_phase2_columns_past_one_grid():
    src, r1cs = SC.columns_past_one_grid_phase2(CU)
    assert r1cs["n_constraints"] == 4096 and r1cs["nb_wires"] == src["n_constraints"] < 2200
    for name in "ABC":
        n_long, n_pieces = RC.split_counts(src, name)
        assert n_long > W1 + 50 and n_pieces > n_long
        lens = np.bincount(r1cs[name][1], minlength=r1cs["nb_wires"])
        assert int((lens == RC.SHORT + 1).sum()) == W1 + 51 and int((lens == RC.CHUNK + 1).sum()) == 2
    # the coefficient mix: most entries take the short paths, some the full double-and-add
    table = [S._int(c) for c in src["coeffs"]]
    small = lambda c: min(c, P.R_MOD - c) < (1 << 32) + 1
    assert [small(c) for c in table] == [True] * 8 + [False] * 4
    share = np.bincount(src["B"][2], minlength=12) / len(src["B"][2])
    assert 0.02 < share[8:].sum() < 0.06 and share[:2].sum() > 0.6


def test_satisfied_system_with_long_rows_in_c():
    r1cs, W, a, b, c = SC.satisfied()
    nc, la, nab = r1cs["n_constraints"], r1cs["long_at"], r1cs["slack0"]
    assert nc == 1061 and nc % 64
    assert sorted(la["A"]) == [0, 1, nc - 1] and sorted(la["B"]) == [nc - 1] and sorted(la["C"]) == [0, nc // 2, nc - 1]
    used = sorted({n for name in "ABC" for n in la[name].values()})
    assert used == [17, 512, 513, 1025]
    for name in "ABC":
        lens = _row_lens(r1cs, name)
        assert {i: int(lens[i]) for i in np.nonzero(lens > RC.SHORT)[0]} == la[name]
        assert RC.split_counts(r1cs, name) == (len(la[name]), sum(-(-n // RC.CHUNK) for n in la[name].values()))
    # the slack wires: once each, as the last entry of their row of C with coefficient 1; the once-only wire in A's third piece
    cols = np.concatenate([r1cs[name][1] for name in "ABC"])
    count = np.bincount(cols, minlength=r1cs["nb_wires"])
    once, row = r1cs["once"]
    assert (count[nab:] == 1).all() and once == r1cs["nb_wires"] - 1 and row == nc - 1
    rp, col, cf = r1cs["C"]
    ends = rp[1:].astype(np.int64) - 1
    assert np.array_equal(col[ends], nab + np.arange(nc)) and (cf[ends] == 1).all() and S._int(r1cs["coeffs"][1]) == 1
    rp, col, cf = r1cs["A"]
    at = int(np.nonzero(col == once)[0][0]) - int(rp[row])
    assert la["A"][row] == 1025 and at >= 2 * RC.CHUNK and S._int(r1cs["coeffs"][cf[int(rp[row]) + at]]) != 0 and S._int(b[row]) != 0
    # the references
    ref = RC.eval_all(r1cs, W)
    for have, want in zip(ref, (a, b, c)):
        assert np.array_equal(have, want)
    for name, have in zip("ABC", ref):
        for i in la[name]:
            assert S._int(have[i]) == RC.row_by_integers(r1cs, name, W, i), f"{name} row {i}"
    assert RC.check_rows(*ref) == (0, RC.U64_MAX)
    sets = SC.bad_row_sets(r1cs)
    assert len(sets) == 6 + 3 + 1 + 3 + 2
    for label, rows in sets:
        W2 = RC.bumped(W, [nab + i for i in rows])
        assert RC.check_rows(*RC.eval_all(r1cs, W2)) == (len(rows), min(rows)), label
    assert RC.check_rows(*RC.eval_all(r1cs, RC.bumped(W, [once]))) == (1, row)
