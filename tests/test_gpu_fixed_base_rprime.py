"""GPU parity for fixed-base MSMs over window tables in the R' form (mi_msm_table_to_rprime_*, MI_MSM_TABLE_RPRIME through the public
mi_msm_g*_fixed_dev: the launch the benchmark's roofline line is quoted on) and for every compile-time window width 17..22: the
conversion word for word, G1 and G2 sums against the C oracle under the sort and level-1 knobs, the item levels, the finisher and the
flat-sort rule on shapes whose histograms (computed here in Python) prove that those paths run, the fused Z digit count at every
width, and what a converted table does once the 29-bit kernels are switched off.  All comparisons are exact."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
from helpers import *
from gpu_common import load_binding
import bytes_cases as BC
import fixed_base_cases as FB

pytestmark = pytest.mark.gpu
MI_EINVAL = -1
RPRIME = 2   # MI_MSM_TABLE_RPRIME


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def real_y():
    Q = BC.twist_point_real_y()
    assert Q is not None and Q[1][1] == 0
    return Q


def _jac_eq(got, want):
    """both normalised: equal limbs, or both infinity (Z == 0)"""
    k = got.shape[0] // 3
    if not want[2 * k:].any():
        return not got[2 * k:].any()
    return np.array_equal(got, want)


def _reset(ctx):
    """every knob this file touches, back to its default"""
    for k, v in (("l1_wg", 4), ("g2_wg", 1), ("l1_waves", 3), ("finisher", 1), ("finisher_max", 0), ("plain_scatter", 0), ("count_per", 0),
                 ("g1_grid_per_cu", 0), ("finisher_min_level", 2), ("z_count_fused", 1), ("flat_item_l1", 0)):
        ctx.set_knob(k, v)
    lib = ctx.lib
    assert lib.mi_debug_set_msm_limb29(ctx.h, 1) == 0 and lib.mi_debug_set_msm_bound_levels(ctx.h, 0) == 0
    assert lib.mi_debug_set_msm_chunk(ctx.h, 0) == 0 and lib.mi_debug_set_msm_group_bits(ctx.h, 0) == 0
    assert lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0


def _vp(ptr):
    return C.c_void_p(ptr)


# ---------------------------------------------------------------------------------------------------- 1. the conversion, word for word
@pytest.mark.parametrize("g2", [False, True])
def test_conversion_of_hand_made_words(ctx, g2):
    """every word of the first n_points rows becomes (w * 32) % p, (0, 0) stays (0, 0), and no row behind n_points changes -- at the
    sizes around the wave and the 256-thread workgroup"""
    k = 4 if g2 else 2
    rows = FB.coord_rows(k, 300, 11 + k)
    want = FB.times32(rows)
    assert want[1] == [0] * k
    for n_points in (1, 63, 64, 65, 256, 257):
        d = ctx.to_dev(FB.words_to_limbs(rows))
        ctx.msm_table_to_rprime(d.ptr, n_points, g2=g2)
        got = FB.limbs_to_words(d.download((len(rows), 4 * k)), k)
        d.free()
        assert got[:n_points] == want[:n_points], n_points
        assert got[n_points:] == rows[n_points:], n_points


@pytest.mark.parametrize("g2,n,c", [(False, 67, 22), (True, 19, 17)])
def test_conversion_of_a_real_table(ctx, g2, n, c):
    """a window table with infinity bases: every row 32 x the original row mod p, the infinity rows untouched"""
    k = 4 if g2 else 2
    pts = cref.gen_g2(n, 4100) if g2 else cref.gen_g1(n, 4101)
    inf = (0, 17, n - 1)
    for i in inf:
        pts[i] = 0
    dp = ctx.to_dev(pts)
    pre = ctx.msm_precompute(dp.ptr, n, c, g2=g2)
    rows = FB.nwin(c) * n
    before = pre.download((rows, 4 * k))
    ctx.msm_table_to_rprime(pre.ptr, rows, g2=g2)
    after = pre.download((rows, 4 * k))
    dp.free(); pre.free()
    assert np.array_equal(before[:n], pts)
    inf_rows = [w * n + i for w in range(FB.nwin(c)) for i in inf]
    assert not before[inf_rows].any() and not after[inf_rows].any()
    assert before[np.setdiff1d(np.arange(rows), inf_rows)].any(axis=1).all()
    assert FB.limbs_to_words(after, k) == FB.times32(FB.limbs_to_words(before, k))


def test_conversion_and_fixed_entry_arguments(ctx):
    lib = ctx.lib
    pts = cref.gen_g1(8, 4200); sc = cref.gen_scalars(8, 4201, 0)
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = ctx.msm_precompute(dp.ptr, 8, 17)
    p2 = ctx.to_dev(cref.gen_g2(8, 4202))
    pre2 = ctx.msm_precompute(p2.ptr, 8, 17, g2=True)
    out = np.zeros(24, np.uint64)
    try:
        for f in (lib.mi_msm_table_to_rprime_g1_dev, lib.mi_msm_table_to_rprime_g2_dev):
            assert f(ctx.h, None, C.c_size_t(0)) == 0                       # nothing to convert
            assert f(ctx.h, None, C.c_size_t(5)) == MI_EINVAL
        for bad in (4, 6, 8, 0x80000000, 0xFFFFFFFC):                       # flags & ~3
            assert lib.mi_msm_g1_fixed_dev(ctx.h, _vp(pre.ptr), _vp(ds.ptr), C.c_size_t(8), C.c_uint32(17), C.c_uint32(bad), out.ctypes.data_as(C.c_void_p)) == MI_EINVAL
            assert lib.mi_msm_g2_fixed_dev(ctx.h, _vp(pre2.ptr), _vp(ds.ptr), C.c_size_t(8), C.c_uint32(17), C.c_uint32(bad), out.ctypes.data_as(C.c_void_p)) == MI_EINVAL
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, 8, 17), cref.msm_g1(pts, sc))   # the same arguments with flags 0 are taken
        # with the 29-bit kernels off there is nothing a converted table could be used for: refused, and the message names the knob
        assert lib.mi_debug_set_msm_limb29(ctx.h, 0) == 0
        before = pre.download((FB.nwin(17) * 8, 8))
        for f, t in ((lib.mi_msm_table_to_rprime_g1_dev, pre), (lib.mi_msm_table_to_rprime_g2_dev, pre2)):
            assert f(ctx.h, _vp(t.ptr), C.c_size_t(8)) == MI_EINVAL
            assert "mi_debug_set_msm_limb29" in lib.mi_last_error(ctx.h).decode()
        assert np.array_equal(pre.download((FB.nwin(17) * 8, 8)), before)   # and nothing was converted
    finally:
        _reset(ctx)
        for d in (dp, ds, pre, p2, pre2):
            d.free()


# ---------------------------------------------------------------------------------------------------- 2. G1 sums on R' tables
_G1 = {}


def _g1_case(n, dist, c):
    """points, scalars and the oracle's sum of a case: computed once, shared, never changed"""
    if (n, dist, c) not in _G1:
        pts, sc = FB.g1_case(n, dist, c)
        _G1[(n, dist, c)] = (pts, sc, cref.msm_g1(pts, sc))
    return _G1[(n, dist, c)]


@pytest.mark.parametrize("n,dist,c,chunk,gbits", FB.G1_CASES)
def test_rprime_table_msm_g1_vs_oracle(ctx, n, dist, c, chunk, gbits):
    """the unconverted table with flags 0 (8 x 32-bit level 1) and the converted one with MI_MSM_TABLE_RPRIME (29-bit level 1): both
    the oracle's sum, at every width, on the wave and slice edges, under forced chunk sizes and group widths"""
    pts, sc, want = _g1_case(n, dist, c)
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = None
    try:
        assert ctx.lib.mi_debug_set_msm_chunk(ctx.h, chunk) == 0 and ctx.lib.mi_debug_set_msm_group_bits(ctx.h, gbits) == 0
        pre = ctx.msm_precompute(dp.ptr, n, c)
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=0), want), "standard table"
        ctx.msm_table_to_rprime(pre.ptr, FB.nwin(c) * n)
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME), want), "R' table"
    finally:
        _reset(ctx)
        for d in (dp, ds, pre):
            if d:
                d.free()


KNOB_SETS = [{}, {"limb29": 2}, {"l1_waves": 2}, {"l1_wg": 1}, {"l1_wg": 4, "g1_grid_per_cu": 3}, {"l1_waves": 2, "l1_wg": 1, "g1_grid_per_cu": 3, "limb29": 2},
             {"count_per": 8, "plain_scatter": 1}, {"count_per": 1}]


@pytest.mark.parametrize("n,dist,c,chunk,gbits", FB.G1_KNOB_CASES)
def test_rprime_table_msm_g1_under_the_level1_knobs(ctx, n, dist, c, chunk, gbits):
    """the R' leg with R'-form and standard-form partial sums (limb29 1 / 2), both builds of the level-1 kernel (l1_waves 3 / 2), one-
    and four-wave workgroups, the default and a tiny resident grid, and the sort's count_per / plain_scatter"""
    pts, sc, want = _g1_case(n, dist, c)
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = None
    try:
        pre = ctx.msm_precompute(dp.ptr, n, c)
        ctx.msm_table_to_rprime(pre.ptr, FB.nwin(c) * n)
        for ks in KNOB_SETS:
            _reset(ctx)
            assert ctx.lib.mi_debug_set_msm_chunk(ctx.h, chunk) == 0 and ctx.lib.mi_debug_set_msm_group_bits(ctx.h, gbits) == 0
            for k, v in ks.items():
                if k == "limb29":
                    assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, v) == 0
                else:
                    ctx.set_knob(k, v)
            assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME), want), ks
    finally:
        _reset(ctx)
        for d in (dp, ds, pre):
            if d:
                d.free()


# ---------------------------------------------------------------------------------------------------- 3. levels, finisher, flat rule
LEVEL_KNOBS = ([{"finisher": v} for v in (0, 1)] + [{"finisher_max": v} for v in (0, 17, 1 << 20)] + [{"finisher_min_level": v} for v in (0, 2)] +
               [{"flat_item_l1": v} for v in (0, 1, 20, 33)] + [{"bound_levels": v} for v in (0, 1)] +
               [{"finisher_min_level": 0, "finisher_max": 1 << 20}, {"finisher": 0, "bound_levels": 1, "limb29": 2}])


def _run_level_knobs(ctx, pts, sc, c, hist):
    n = pts.shape[0]
    want = cref.msm_g1(pts, sc)
    entries = int(hist.sum())
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = None
    try:
        pre = ctx.msm_precompute(dp.ptr, n, c)
        ctx.msm_table_to_rprime(pre.ptr, FB.nwin(c) * n)
        for ks in LEVEL_KNOBS:
            _reset(ctx)
            for k, v in ks.items():
                if k == "bound_levels":
                    assert ctx.lib.mi_debug_set_msm_bound_levels(ctx.h, v) == 0
                elif k == "limb29":
                    assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, v) == 0
                else:
                    ctx.set_knob(k, v)
            assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME), want), ks
            st = ctx.stats()
            # one level-1 addition per sorted entry = per non-zero digit of the Python recoding
            assert st["g1_level1_additions"] == entries and st["g1_accum_entries"] == entries and st["g1_accum_pairs"] == n, (ks, st)
    finally:
        _reset(ctx)
        for d in (dp, ds, pre):
            if d:
                d.free()


def test_item_levels_and_finisher_on_a_skewed_rprime_table(ctx):
    """n = 70000, c = 17, every third scalar 1: bucket 0 holds a third of the scalars and needs at least three accumulate passes (asserted
    on the Python histogram), so the upper levels in both partial-sum forms, the finisher at every place and the worst-case level count run"""
    pts, sc, c = FB.skewed_shape()
    hist = FB.bucket_histogram(sc, c)
    assert hist[0] > 20000 and FB.item_levels(int(hist.max())) >= 3 and FB.item_levels(int(hist.max()), 32) >= 3
    _run_level_knobs(ctx, pts, sc, c, hist)


@pytest.mark.parametrize("n", [FB.FLAT_N, FB.FLAT_N_RULE])
def test_flat_sort_rule_on_an_rprime_table(ctx, n):
    """uniform scalars, c = 17: the fullest of the 2^16 buckets holds at most twice the average (asserted on the Python histogram).  At
    n = 2^17 the average is 30; msm_accum_enqueue's rule also asks for an average of 64, so the second shape (n = 9 x 2^16, average 134)
    is the one on which the automatic size (17) and the forced sizes 20 and 33 replace the plan's 16"""
    pts, sc, c = FB.flat_shape(n)
    hist = FB.bucket_histogram(sc, c)
    avg = int(hist.sum()) // len(hist)
    assert int(hist.max()) <= 2 * avg
    if n == FB.FLAT_N_RULE:
        assert avg >= 64 and 17 <= -(-avg // FB.ITEM_L2) <= 32
    _run_level_knobs(ctx, pts, sc, c, hist)


# ---------------------------------------------------------------------------------------------------- 4. G2
@pytest.mark.parametrize("n,c", FB.G2_CASES)
def test_rprime_table_msm_g2_vs_oracle(ctx, real_y, n, c):
    """G2 tables, standard and R', one- and four-wave workgroups: repeated and opposite points, an infinity base, and a twist point whose
    y has a zero imaginary part under scalars with negative digits (the per-component negation of the packed words)"""
    pts, sc = FB.g2_case(n, c, real_y)
    want = cref.msm_g2(pts, sc)
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = None
    try:
        pre = ctx.msm_precompute(dp.ptr, n, c, g2=True)
        assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=0, g2=True), want), "standard table"
        ctx.msm_table_to_rprime(pre.ptr, FB.nwin(c) * n, g2=True)
        for wg in (1, 4):
            ctx.set_knob("g2_wg", wg)
            assert _jac_eq(ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME, g2=True), want), ("R' table", wg)
    finally:
        _reset(ctx)
        for d in (dp, ds, pre):
            if d:
                d.free()


@pytest.mark.parametrize("n", [1000, 1 << 14])
def test_generic_msm_g2_with_a_real_y_point(ctx, real_y, n):
    """the same point through the public mi_msm_g2 below and at 2^14 pairs (from where it takes the 29-bit level-1 kernel)"""
    pts, sc = FB.g2_generic_case(n, 4300 + n, real_y)
    want = cref.msm_g2(pts, sc)
    try:
        for wg in (1, 4):
            ctx.set_knob("g2_wg", wg)
            assert _jac_eq(ctx.msm_g2(pts, sc), want), wg
    finally:
        _reset(ctx)
    Q = g2_arr([real_y, real_y, real_y])
    vals = [P.R_MOD - 1, (1 << 15) - 1, 5]
    assert g2_from_jac(ctx.msm_g2(Q, fr_arr(vals))) == P.g2_mul(real_y, sum(vals))


# ---------------------------------------------------------------------------------------------------- 5. the fused Z count, every width
def _prove_case(log_n, seed):
    N = 1 << log_n
    nw, nc = N - 37, N - 5
    pk = synthetic_pk(log_n, nw, 40, seed)
    W = cref.gen_scalars(nw, 1, 1); a = cref.gen_scalars(nc, 2, 0); b = cref.gen_scalars(nc, 3, 0); c = cref.field_op(0, 2, a, b)
    r, s = cref.gen_scalars(2, 4, 0)
    return pk, W, a, b, c, r, s, cref.proof_write(cref.prove(pk, W, a, b, c, r, s)["raw"])


@pytest.mark.parametrize("log_n,widths", [(13, FB.WIDTHS), (16, (21,))])
def test_z_digit_count_from_compute_h_at_every_window_width(ctx, log_n, widths):
    """computeH's last launch counts the Z MSM's digits in an instantiation of its own per window width (a different limb-straddling
    path each): proofs with the fused count and with the sort's own count pass, c given and formed on the device, equal the oracle's
    bytes at every width, and the counter shows that the fused launch ran exactly for the fused proofs"""
    B = load_binding()
    pk, W, a, b, c, r, s, want = _prove_case(log_n, 7300 + log_n)
    try:
        for cz in widths:
            assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 17, 17, cz) == 0
            pkh = ctx.pk_load(pk)
            assert ctx.pk_table_plan(pkh)[2] == cz
            for fused in (1, 0):
                ctx.set_knob("z_count_fused", fused)
                before = ctx.counter("z_count_fused_launches")
                got, _ = ctx.prove(pkh, W, a, b, c, r, s)
                assert B.proof_write(got["raw"]) == want, (cz, fused, "c given")
                got, _ = ctx.prove(pkh, W, a, b, None, r, s)
                assert B.proof_write(got["raw"]) == want, (cz, fused, "c formed on the device")
                assert ctx.counter("z_count_fused_launches") == before + 2 * fused, (cz, fused)
            ctx.pk_free(pkh)
    finally:
        _reset(ctx)


# ---------------------------------------------------------------------------------------------------- 6. a converted table, 29-bit kernels off
@pytest.mark.parametrize("g2", [False, True])
def test_converted_table_with_the_29_bit_kernels_switched_off(ctx, real_y, g2):
    """mi_debug_set_msm_limb29(0) after the conversion: MI_MSM_TABLE_RPRIME still selects the 29-bit level 1 (choose_level1 looks at the
    flag, not at the knob; the 8 x 32-bit kernel never meets the converted words), so the sum is the oracle's.  A refusal with a message
    would be as good; a wrong sum is the bug"""
    B = load_binding()
    n, c = 3000, 18
    if g2:
        pts, sc = FB.g2_case(n, c, real_y); want = cref.msm_g2(pts, sc)
    else:
        pts, sc, want = _g1_case(5000, 0, 18); n = 5000
    dp, ds = ctx.to_dev(pts), ctx.to_dev(sc)
    pre = None
    try:
        pre = ctx.msm_precompute(dp.ptr, n, c, g2=g2)
        ctx.msm_table_to_rprime(pre.ptr, FB.nwin(c) * n, g2=g2)
        assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, 0) == 0
        try:
            got = ctx.msm_fixed_dev(pre.ptr, ds.ptr, n, c, flags=RPRIME, g2=g2)
        except B.MiError as e:
            assert f"rc={MI_EINVAL}:" in str(e) and "mi_debug_set_msm_limb29" in str(e)
        else:
            assert _jac_eq(got, want)
    finally:
        _reset(ctx)
        for d in (dp, ds, pre):
            if d:
                d.free()
