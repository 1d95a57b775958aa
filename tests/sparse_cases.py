"""The cases of tests/test_gpu_sparse_sums.py, built from the generators of tests/r1cs_cases.py and checked on the CPU by
tests/test_sparse_cases_cpu.py, so that no GPU test passes because its input missed the path it is there for.

The wave passes of the split sum (csrc/sparse_fr.cuh, csrc/sparse_points.cuh) run on a capped grid and stride over their work: Setup and
the resident R1CS launch at most 8 blocks of four waves per CU (waves4 = 32 CU waves), phase 2 at most 8 single-wave workgroups per CU
(waves1 = 8 CU).  A pass takes a second trip of its loop only with more long lists, or pieces, than that.
"""
import numpy as np
import pyref as P
import cref
import r1cs_cases as RC
from helpers import fr_arr

R = P.R_MOD


def waves4(cu):
    return 32 * cu


def waves1(cu):
    return 8 * cu


# the heavy matrix -> the roles of A, B, C: every matrix is once the one with thousands of long rows, once the one with one, once with none
ROLES = {"A": (RC.HEAVY, RC.ONE, RC.NONE), "B": (RC.NONE, RC.HEAVY, RC.ONE), "C": (RC.ONE, RC.NONE, RC.HEAVY)}
N_DOUBLE, ONE_LEN = 40, 2 * RC.CHUNK + 1


def rows_past_one_grid(cu, heavy):
    """waves4 + 150 rows of 17 entries and 40 of 513 in the matrix `heavy`, one row of 1025 in the next, no long row in the third; about
    9000 constraints at 256 CUs, over 4096 wires (so the transposed system has 2^12 constraints)"""
    return RC.many_long_r1cs(waves4(cu) + 150, roles=ROLES[heavy], nb_wires=4096, nb_public=33, seed=3100 + "ABC".index(heavy), n_double=N_DOUBLE,
                             one_len=ONE_LEN)


def rows_counts(cu):
    """(long rows, pieces) of rows_past_one_grid's heavy, one and none matrix"""
    n = waves4(cu) + 150
    return {RC.HEAVY: (n + N_DOUBLE, n + 2 * N_DOUBLE), RC.ONE: (1, 3), RC.NONE: (0, 0)}


def pinned_rows(r1cs, cu):
    """the rows to make bad one at a time in rows_past_one_grid made solvable (r1cs_cases.with_slack): the heavy matrix's long rows at the
    places 0, 32 CU - 1, 32 CU (the first a wave reaches on its second trip) and the last of its list of long rows, which the library
    keeps ascending by row; the one long row of the second matrix; and a short row"""
    heavy = "ABC"[r1cs["roles"].index(RC.HEAVY)]
    rows = np.sort(r1cs["planted"][heavy][0])
    one = r1cs["planted"]["ABC"[r1cs["roles"].index(RC.ONE)]][0]
    short = next(i for i in range(r1cs["n_constraints"]) if all(r1cs["lens"][n][i] <= RC.SHORT for n in "ABC"))
    return [int(rows[0]), int(rows[waves4(cu) - 1]), int(rows[waves4(cu)]), int(rows[-1]), int(one[0]), short]


# phase 2: coefficient 1 and r - 1 are a mixed addition, c or r - c below 2^32 a short multiplication, the rest a double-and-add over 254 bits
_PHASE2_SMALL = [1, R - 1, 2, R - 2, 3, (1 << 32) - 1, 1 << 32, R - (1 << 32)]
PHASE2_SHARES = [.36, .36] + [.04] * 6 + [.01] * 4      # 4 % of the entries are full width


def phase2_coeffs():
    return np.concatenate([fr_arr(_PHASE2_SMALL), cref.gen_scalars(4, 3207, 0)])


def columns_past_one_grid_phase2(cu):
    """(src, its transpose): waves1 + 51 columns of 17 entries and two of 513 in EACH of A, B and C, over 2^12 constraints"""
    n = waves1(cu) + 51
    src = RC.many_long_r1cs(n, roles=(RC.HEAVY,) * 3, n_constraints=n + 2 + 47, nb_wires=4096, nb_public=9, seed=3200, n_double=2,
                            coeffs=phase2_coeffs(), shares=PHASE2_SHARES)
    return src, RC.transposed(src)


def satisfied():
    return RC.satisfied_r1cs_long_c(n_constraints=1061, nb_wires_ab=700, nb_public=9, seed=3300)


def bad_row_sets(r1cs):
    """[(label, rows)]: adding 1 to the slack wires of `rows` must give (len(rows), min(rows))"""
    nc, la = r1cs["n_constraints"], r1cs["long_at"]
    sets = [("row 0", {0}), ("row 63", {63}), ("row 64", {64}), ("rows 255, 256", {255, 256}), ("the last row", {nc - 1}), ("the last row and row 0", {nc - 1, 0})]
    for name in "ABC":
        sets += [(f"{name}'s long row {row} ({n} entries)", {row}) for row, n in sorted(la[name].items())]
    in_all = set(la["A"]) & set(la["B"]) & set(la["C"])
    assert len(in_all) == 1
    sets += [("the row long in A, B and C", in_all), ("all rows", set(range(nc)))]
    return sets
