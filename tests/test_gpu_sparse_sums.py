"""GPU: the split sum of skewed lists (csrc/sparse_fr.cuh, csrc/sparse_points.cuh) past one grid of waves, under unequal plans in one
launch and after a larger call on the same context, in its three callers (csrc/setup.hip, csrc/r1cs.hip, csrc/phase2.hip); and the
constraint check pinned to single rows.  Every comparison is exact, against the host references of tests/r1cs_cases.py and
tests/setup_cases.py; phase 2 against mi_groth16_setup_to_streams (the yardstick of tests/test_gpu_phase2.py).

The inputs are tests/sparse_cases.py's, sized by the device's CU count and checked on the CPU for 256 CUs by
tests/test_sparse_cases_cpu.py.  Each test asserts its path condition on the counts the library itself reports.

1  R1CS rows: more long rows and more pieces than the 32 CU waves of the capped grid in one matrix, one long row in the second, none in
   the third, each matrix in each role, every `which`, host and device entry points; the same system made solvable, so that the
   check's compact combine past one grid is pinned too
2  Setup columns: the transpose of the same system
3  phase-2 point sums: more long columns than the 8 CU single-wave workgroups in each of A, B, C
4  the check: a satisfied system with long rows in A, B and C; one bad row at a chosen place gives exactly (1, that row)
5  a large plan, then a small one, on one context without a trim

Measured on an MI355X (256 CUs: 8383 long rows and 8425 pieces against 8192 waves; 6303 long columns over the three phase-2 plans
against 2048), pytest's duration of each test with its inputs and host references: the R1CS rows and the check past one grid 0.03 to
0.04 s per role, Setup past one grid and then the split edges 0.67 s, phase 2 past one grid 0.68 s (phase2_init itself 0.61 s), the
pinned check and large-then-small on the R1CS under 0.01 s each, phase 2 large then small 1.33 s; the whole file 3.3 s from its first
test to its last, 5.4 s with collection.  One mutation of the library at a time (not committed): the wave loops of sparse_sum_pieces
and sparse_combine cut to one trip fails sections 1, 2 and 5; the same in sparse_points.cuh fails section 3 and phase 2's part of 5;
`<` for `<=` in row_value's search, and the compact combine storing to index % n_long, each fail section 4, the check of 1 and 5.
"""
import time
import numpy as np
import pytest
import torch
import setup_cases as S
import r1cs_cases as RC
import sparse_cases as SC
from gpu_common import load_binding
from test_gpu_setup import split_edge_wires
from test_gpu_phase2 import make_srs, secrets, trapdoor, assert_equals_setup, RAW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    t0 = time.perf_counter()
    c = B.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_sparse_sums.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


@pytest.fixture(scope="module")
def cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Timer:
    def __init__(self, what):
        self.what, self.t0 = what, time.perf_counter()

    def done(self, *stats):
        print(f"\n{self.what}: {time.perf_counter() - self.t0:.2f} s wall; " + "; ".join(str(s) for s in stats))


_rows_cache = {}


def _rows_case(cu, heavy):
    """(r1cs, W, (A W, B W, C W) by the host reference) of sparse_cases.rows_past_one_grid, made once"""
    if (cu, heavy) not in _rows_cache:
        r1cs = SC.rows_past_one_grid(cu, heavy)
        W = RC.witness(r1cs["nb_wires"], 3110 + "ABC".index(heavy))
        ref = RC.eval_all(r1cs, W)
        for x in ref:
            x.setflags(write=False)
        _rows_cache[(cu, heavy)] = (r1cs, W, ref)
    return _rows_cache[(cu, heavy)]


@pytest.fixture(scope="module")
def small():
    """sparse_cases.satisfied(): (r1cs, W, a, b, c)"""
    return SC.satisfied()


def _names(which):
    return "".join(n for k, n in enumerate("ABC") if which & (1 << k))


def _assert_eval(ctx, rh, r1cs, W, ref, which, device, what):
    """one evaluation of the matrices in `which` against ref, and the stats against the plan of those matrices; returns the stats"""
    n = r1cs["n_constraints"]
    got = ctx.r1cs_eval(rh, W, n, which=which, device=device)
    st = ctx.r1cs_stats()
    names = _names(which)
    for k, name in enumerate("ABC"):
        if name in names:
            assert np.array_equal(got[k], ref[k]), f"{what}: {name} W, which = {which}, {'device' if device else 'host'} entry point"
        else:
            assert got[k] is None
    assert (st["matrices"], st["entries"], st["long_rows"], st["pieces"]) == (len(names), sum(len(r1cs[m][1]) for m in names)) + RC.split_counts(r1cs, names), f"{what}: which = {which}"
    return st


# ---------------------------------------------------------------------------------------------------- 1: R1CS rows past one grid
@pytest.mark.parametrize("heavy", "ABC")
def test_r1cs_rows_past_one_grid(ctx, cu, heavy):
    """every `which` (B | C puts B in slot 0 of the launch; a matrix with no long row beside one with thousands), both entry points.
    The grid of the two wave passes is sized by the largest requested matrix: with the heavy matrix requested both passes take a
    second trip of their loops (long_rows > 32 CU and pieces > 32 CU); without it the call has one long row or none."""
    r1cs, W, ref = _rows_case(cu, heavy)
    w4 = SC.waves4(cu)
    t = _Timer(f"r1cs rows past one grid, heavy {heavy}")
    rh = ctx.r1cs_load(r1cs)
    dW = ctx.to_dev(W)
    try:
        past = 0
        for which in range(1, 8):
            for device in (False, True):
                st = _assert_eval(ctx, rh, r1cs, dW.ptr if device else W, ref, which, device, f"heavy {heavy}")
                if heavy in _names(which):
                    assert st["long_rows"] > w4 and st["pieces"] > w4, (st, w4)
                    past += 1
                else:
                    assert st["long_rows"] <= 1
        assert past == 2 * 4
        # the check runs the compact combine over the same plan
        assert ctx.r1cs_check(rh, dW.ptr, device=True) == RC.check_rows(*ref)
        st = ctx.r1cs_stats()
        assert st["matrices"] == 3 and (st["long_rows"], st["pieces"]) == RC.split_counts(r1cs) and st["long_rows"] > w4
        t.done(st, f"32 CU = {w4}")
    finally:
        dW.free()
        ctx.r1cs_free(rh)


@pytest.mark.parametrize("heavy", "ABC")
def test_r1cs_check_past_one_grid(ctx, cu, heavy):
    """the same system made solvable (one slack wire per row of C): the check's compact combine takes its second trip, and a wrong or
    missing sum of any long row shows, since no row is bad.  Then one bad row at a time: the first and the last long row, the last of
    the first trip and the first of the second, the second matrix's one long row, a short row."""
    src, W0, _ = _rows_case(cu, heavy)
    r1cs, W, a, b, c = RC.with_slack(src, W0)
    t = _Timer(f"r1cs check past one grid, heavy {heavy}")
    rh = ctx.r1cs_load(r1cs)
    dW = ctx.to_dev(W)
    try:
        _assert_eval(ctx, rh, r1cs, W, (a, b, c), 7, False, f"solvable, heavy {heavy}")
        assert ctx.r1cs_check(rh, dW.ptr, device=True) == (0, RC.U64_MAX)
        st = ctx.r1cs_stats()
        assert (st["matrices"], st["long_rows"], st["pieces"]) == (3,) + RC.split_counts(src) and st["long_rows"] > SC.waves4(cu)
        for i in SC.pinned_rows(src, cu):
            assert ctx.r1cs_check(rh, RC.bumped(W, [r1cs["slack0"] + i])) == (1, i), f"row {i}"
        assert ctx.r1cs_check(rh, W) == (0, RC.U64_MAX)
        t.done(st)
    finally:
        dW.free()
        ctx.r1cs_free(rh)


# ---------------------------------------------------------------------------------------------------- 2: Setup columns past one grid
def _setup_many_long(ctx, cu):
    """setup_exponents of the transpose of rows_past_one_grid(heavy A): every planted column in integers, every matrix by the identity"""
    src, _, _ = _rows_case(cu, "A")
    r1cs = RC.transposed(src)
    td = S.synth_trapdoor(3120)
    got = ctx.setup_exponents(r1cs, td)
    st = ctx.setup_stats()
    assert (st["long_columns"], st["chunks"]) == RC.split_counts(src) and st["entries"] == sum(len(r1cs[m][1]) for m in "ABC")
    assert st["long_columns"] > SC.waves4(cu) and st["chunks"] > SC.waves4(cu), (st, cu)
    RC.check_columns(r1cs, td, got, {name: src["planted"][name][0] for name in "ABC"}, seed=3121)
    S.check_z(td, 12, got["z"])
    return st


def _setup_split_edges(ctx):
    """the system of test_gpu_setup.py::test_setup_columns_at_the_split_edges with its checks"""
    src = RC.skewed_r1cs(n_constraints=3000, nb_wires=4096, nb_public=33, seed=1208)
    r1cs = RC.transposed(src)
    td = S.synth_trapdoor(1209)
    got = ctx.setup_exponents(r1cs, td)
    st = ctx.setup_stats()
    assert (st["long_columns"], st["chunks"]) == RC.split_counts(src)
    RC.check_columns(r1cs, td, got, split_edge_wires(src, r1cs), seed=1210)
    S.check_z(td, 12, got["z"])
    return st


def test_setup_columns_past_one_grid_then_the_split_edges(ctx, cu):
    """more long columns than 32 CU: k_col_sum_combine and k_col_sum_pieces stride; then, on the same context, the small plan of the
    split-edge system (the counters and the partials of the large call are behind it)"""
    t = _Timer("setup_exponents past one grid")
    big = _setup_many_long(ctx, cu)
    t.done(big)
    t = _Timer("setup_exponents at the split edges after it")
    t.done(_setup_split_edges(ctx))


# ---------------------------------------------------------------------------------------------------- 3: phase-2 point sums past one grid
@pytest.fixture(scope="module")
def p2big(ctx, cu):
    src, r1cs = SC.columns_past_one_grid_phase2(cu)
    tau, alpha, beta, _ = secrets(3130)
    return dict(src=src, r1cs=r1cs, srs=make_srs(ctx, r1cs["n_constraints"], tau, alpha, beta), td=trapdoor(tau, alpha, beta))


def _phase2_past_one_grid_stats(ctx, cu, g):
    stats = ctx.phase2_stats()
    w1 = SC.waves1(cu)
    per = [RC.split_counts(g["src"], name) for name in "ABC"]
    assert all(n_long > w1 + 50 and n_pieces > w1 + 50 for n_long, n_pieces in per), (per, w1)
    # the library reports the plan of the sum that takes all three matrices: its counts are the three plans added up
    assert (stats["long_columns"], stats["chunks"]) == RC.split_counts(g["src"]) and stats["long_columns"] > 3 * (w1 + 50), (stats, w1)
    assert stats["entries"] == sum(len(g["r1cs"][m][1]) for m in "ABC")
    return stats


def test_phase2_point_sums_past_one_grid(ctx, cu, p2big):
    """more long columns than 8 CU in each of A, B and C: sparse_points_pieces and sparse_points_combine stride in the G1 sums of A, of B
    and of the three pairs of t, and in the G2 sum of B.  Both encodings of both streams against Setup's."""
    g = p2big
    assert g["r1cs"]["n_constraints"] <= 4096
    t = _Timer("phase2_init past one grid")
    st = ctx.phase2_init(g["r1cs"], g["srs"])
    try:
        stats = _phase2_past_one_grid_stats(ctx, cu, g)
        assert_equals_setup(ctx, g["r1cs"], st, g["td"])
        t.done(stats, f"8 CU = {SC.waves1(cu)}")
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 4: the check, pinned
def test_r1cs_check_pins_single_rows(ctx, small):
    """long rows in A, B and C of a satisfied system of 1061 constraints (not a multiple of 64): the check reads C's compact sums and
    finds each long row by binary search among 3, 1 and 3 of them.  One bad row at a chosen place gives exactly (1, that row)."""
    r1cs, W, a, b, c = small
    nab = r1cs["slack0"]
    t = _Timer("r1cs_check pinned")
    rh = ctx.r1cs_load(r1cs)
    try:
        for have, want, name in zip(ctx.r1cs_eval(rh, W, r1cs["n_constraints"]), (a, b, c), "abc"):
            assert np.array_equal(have, want), name
        assert ctx.r1cs_check(rh, W) == (0, RC.U64_MAX)
        st = ctx.r1cs_stats()
        assert (st["matrices"], st["long_rows"], st["pieces"]) == (3,) + RC.split_counts(r1cs) == (3, 7, 6 + 1 + 5)
        once, row = r1cs["once"]
        cases = [(label, RC.bumped(W, [nab + i for i in rows]), (len(rows), min(rows))) for label, rows in SC.bad_row_sets(r1cs)]
        cases.append(("the wire that occurs once, in the third piece of A's last row", RC.bumped(W, [once]), (1, row)))
        for label, W2, want in cases:
            assert ctx.r1cs_check(rh, W2) == want, f"{label} (host pointer)"
        for label, W2, want in cases[:3] + cases[6:10] + cases[-3:]:
            dW = ctx.to_dev(W2)
            try:
                assert ctx.r1cs_check(rh, dW.ptr, device=True) == want, f"{label} (device pointer)"
            finally:
                dW.free()
        assert ctx.r1cs_check(rh, W) == (0, RC.U64_MAX)
        t.done(st, f"{len(cases)} wire vectors")
    finally:
        ctx.r1cs_free(rh)


# ---------------------------------------------------------------------------------------------------- 5: large, then small
def test_r1cs_large_then_small_on_one_context(ctx, cu, small):
    """WS_R1CS_PARTIAL and the check's workspace grow with the large system and are never cleared: the small system's sums and its
    check must not read what the large one left there, and the other way round.  No trim in between."""
    B = load_binding()
    big, bigW, big_ref = _rows_case(cu, "A")
    r1cs, W, a, b, c = small
    nab, nc = r1cs["slack0"], r1cs["n_constraints"]
    t = _Timer("r1cs large, small, large, small")
    rh_big, rh = ctx.r1cs_load(big), ctx.r1cs_load(r1cs)
    try:
        for which in (7, B.R1CS_B | B.R1CS_C):
            st = _assert_eval(ctx, rh_big, big, bigW, big_ref, 7, False, "large")
            assert st["long_rows"] > SC.waves4(cu) and st["pieces"] > SC.waves4(cu)
            assert ctx.r1cs_check(rh_big, bigW) == RC.check_rows(*big_ref)
            _assert_eval(ctx, rh, r1cs, W, (a, b, c), which, False, "small after large")
            assert ctx.r1cs_check(rh, W) == (0, RC.U64_MAX)
            for rows in ({nc - 1}, {0, nc // 2}):
                assert ctx.r1cs_check(rh, RC.bumped(W, [nab + i for i in rows])) == (len(rows), min(rows))
        t.done(ctx.r1cs_stats())
    finally:
        ctx.r1cs_free(rh); ctx.r1cs_free(rh_big)


def test_phase2_large_then_small_on_one_context(ctx, cu, p2big):
    """phase2_init of the many-long system, then of a 100-constraint one on the same context, compared with Setup: the plan's counters
    are zero again before the short pass, and nothing of the large plan is read"""
    g = p2big
    t = _Timer("phase2_init large, then small")
    st = ctx.phase2_init(g["r1cs"], g["srs"])
    try:
        big_stats = _phase2_past_one_grid_stats(ctx, cu, g)
        assert_equals_setup(ctx, g["r1cs"], st, g["td"], encodings=(RAW,))
    finally:
        ctx.phase2_free(st)
    nc = 100
    tau, alpha, beta, _ = secrets(3140)
    r1cs = S.synth_r1cs(nc, nb_wires=140, nb_public=5, seed=3141, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=40, n_empty_cols=6)
    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, tau, alpha, beta))
    try:
        stats = ctx.phase2_stats()
        assert stats["entries"] == sum(len(r1cs[m][1]) for m in "ABC") and 0 < stats["long_columns"] < 16
        assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta))
        t.done(big_stats, stats)
    finally:
        ctx.phase2_free(st)
