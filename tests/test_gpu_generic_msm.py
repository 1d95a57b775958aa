"""GPU parity for the generic Pippenger path (msm_sort_enqueue in csrc/msm.hip): every window width 2..16 with the signed-digit edge
scalars of that width, both sides of the two places where the sort changes (auto_c reaching 16 at 2^20 pairs, and c = 16 meeting 2^18
pairs), and the degenerate scalar sets -- an empty sort, one entry, every entry in one key -- on both sorts.  Every sum is compared exactly
with the oracle's (cref.msm_g1 / msm_g2; a size that extends another by a few pairs takes the oracle's sum of those pairs and the oracle's
addition, generic_msm_cases.oracle_plus).  Inputs: tests/generic_msm_cases.py, proven by tests/test_generic_msm_cpu.py.

  a  every width, small: the edge scalars of the width, G1 and G2, Montgomery and canonical scalars
  b  every width at 2^16 + 37 (G1) / 2^14 + 37 (G2) pairs, just above the sizes from which the bases are converted to the R' form: the
     29-bit level 1 at every width; the other two limb modes and the two-wave build at c = 2, 9, 16
  c  n = 2^k - 1 and 2^k with no knob: the widths auto_c gives, and by counter which sort ran
  d  c = 16 around 2^18 pairs: by counter which sort ran, both sorts from 2^18 on
  e  degenerate sets of 2^18 pairs at c = 16 on both sorts, with counted and worst-case item levels; three of them at 2^20 with no knob
  f  degenerate sets of 3000 pairs at c = 3, 8, 13

Wall time of this file on an MI355X, printed at the end of the run: 5.0 s for its 99 cases inside a whole GPU suite of 650 s (the 666 older
cases take the other 645 s), so nothing of (b) or (e) was cut.  The large point vectors come from the device's generator; the oracle's own
would take 9 s for 2^18 G2 points.  Two notes on the inputs: for 2^7 and 2^8 pairs the edge
scalars of both widths do not fit the vector, so generic_msm_cases.planted_scalars keeps the ones that reach the four digit edges of each
width and fills the room with the others in turn; and the set `all_min_digits_16` holds the value whose every digit IS -2^15 at c = 16,
while sum_k 2^15 << 16 k (digits -2^15, then -(2^15 - 1)) is a set of its own, `all_half_chunks_16`."""
import time
import numpy as np
import pytest
import cref
import fixed_base_cases as FB
import generic_msm_cases as GM
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
N18 = GM.SORT_SWITCH


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    t0 = time.perf_counter()
    c = B.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_generic_msm.py: {time.perf_counter() - t0:.1f} s wall from its first test to its last")


def _reset(ctx):
    lib = ctx.lib
    assert lib.mi_debug_set_msm_plan(ctx.h, 0, 0, 0, 0, 0) == 0 and lib.mi_debug_set_msm_limb29(ctx.h, 1) == 0
    assert lib.mi_debug_set_msm_l1_waves(ctx.h, 3) == 0 and lib.mi_debug_set_msm_one_pass_sort(ctx.h, 0) == 0
    assert lib.mi_debug_set_msm_bound_levels(ctx.h, 0) == 0


def _width(ctx, c):
    assert ctx.lib.mi_debug_set_msm_plan(ctx.h, c, 0, 0, 0, 0) == 0


def _device_points(ctx):
    """the device's point generator for the large vectors (generic_msm_cases checks what it returns against the curve equation)"""
    def gen(n, seed, g2):
        d = (ctx.gen_g2 if g2 else ctx.gen_g1)(n, seed)
        out = d.download((n, 16 if g2 else 8))
        d.free()
        return out
    return gen


def _sorts(ctx):
    return ctx.counter("generic_sorts_one_pass"), ctx.counter("generic_sorts_two_pass")


class _Resident:
    """points, Montgomery and canonical scalars of one case on the device: every size and knob runs on prefixes of the same arrays"""
    def __init__(self, ctx, pts, sc, g2):
        self.ctx, self.g2, self.pts, self.sc, self.n = ctx, g2, pts, sc, pts.shape[0]
        self.dev = [ctx.to_dev(pts), ctx.to_dev(sc), ctx.to_dev(FB.canonical(sc))]

    def msm(self, n=None, canonical=False):
        f = self.ctx.msm_g2_dev if self.g2 else self.ctx.msm_g1_dev
        return f(self.dev[0].ptr, self.dev[2 if canonical else 1].ptr, self.n if n is None else n, flags=1 if canonical else 0)

    def oracle(self, n=None):
        n = self.n if n is None else n
        return (cref.msm_g2 if self.g2 else cref.msm_g1)(self.pts[:n], self.sc[:n])

    def free(self):
        for d in self.dev:
            d.free()


# ---------------------------------------------------------------------------------------------------- a: every width, small
@pytest.mark.parametrize("c", GM.WIDTHS)
def test_every_width_on_its_edge_scalars(ctx, c):
    """300 planted pairs, the edge scalars of width c and a ragged end, with the width forced: G1, and G2 points under the same scalars;
    Montgomery scalars and canonical ones (flags = 1)"""
    n = GM.small_n(c)
    pts, sc = GM.case(n, [c], False, 5000 + c)
    p2, _ = GM.case(n, [c], True, 5100 + c)        # (its plants sit where the G1 case's do: the scalars of the G1 case serve both)
    canon = FB.canonical(sc)
    want1, want2 = cref.msm_g1(pts, sc), cref.msm_g2(p2, sc)
    assert want1[8:].any() and want2[16:].any()
    try:
        _width(ctx, c)
        before = _sorts(ctx)
        for s, flags in ((sc, 0), (canon, 1)):
            assert np.array_equal(ctx.msm_g1(pts, s, flags=flags), want1), (c, flags)
            assert np.array_equal(ctx.msm_g2(p2, s, flags=flags), want2), (c, flags)
        assert _sorts(ctx) == (before[0] + 4, before[1])
    finally:
        _reset(ctx)


# ---------------------------------------------------------------------------------------------------- b: every width, 29-bit level 1
@pytest.fixture(scope="module")
def all_widths(ctx):
    """one G1 vector of 2^16 + 37 pairs and one G2 vector of 2^14 + 37 that carry the edge scalars of all fifteen widths: one oracle
    sum per curve serves every width and every mode"""
    gen = _device_points(ctx)
    g1 = _Resident(ctx, *GM.case((1 << 16) + 37, GM.WIDTHS, False, 5200, gen=gen), False)
    g2 = _Resident(ctx, *GM.case((1 << 14) + 37, GM.WIDTHS, True, 5300, gen=gen), True)
    yield g1, g1.oracle(), g2, g2.oracle()
    g1.free(); g2.free()


@pytest.mark.parametrize("c", GM.WIDTHS)
def test_every_width_under_the_29_bit_level1(ctx, all_widths, c):
    """c = 2 is 128 windows of two buckets with some 2^15 entries each (deep item levels), c = 16 the one-pass sort with its 128 KiB
    histogram"""
    g1, want1, g2, want2 = all_widths
    try:
        _width(ctx, c)
        assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, 1) == 0
        assert np.array_equal(g1.msm(), want1), c
        assert np.array_equal(g2.msm(), want2), c
        assert np.array_equal(g1.msm(canonical=True), want1), c
    finally:
        _reset(ctx)


@pytest.mark.parametrize("c", [2, 9, 16])
def test_narrowest_middle_and_widest_width_in_the_other_level1_builds(ctx, all_widths, c):
    """standard-form partial sums after a 29-bit level 1 (2), 8 x 32-bit limbs throughout (0), and the two-waves-per-SIMD build"""
    g1, want1, g2, want2 = all_widths
    try:
        _width(ctx, c)
        for limb29, waves in ((2, 3), (0, 3), (1, 2)):
            assert ctx.lib.mi_debug_set_msm_limb29(ctx.h, limb29) == 0 and ctx.lib.mi_debug_set_msm_l1_waves(ctx.h, waves) == 0
            assert np.array_equal(g1.msm(), want1), (c, limb29, waves)
            assert np.array_equal(g2.msm(), want2), (c, limb29, waves)
    finally:
        _reset(ctx)


# ---------------------------------------------------------------------------------------------------- c: where auto_c switches
def _auto_c_switch(ctx, k, g2):
    n = 1 << k
    cs = [GM.auto_c(n - 1), GM.auto_c(n)]
    assert cs == [max(3, k - 5), k - 4]            # (k = 7: both sizes run at the lower clamp, 3)
    pts, sc = GM.case(n, cs, g2, 6000 + 100 * g2 + k, gen=_device_points(ctx) if k >= 14 else None)
    msm, run = (cref.msm_g2, ctx.msm_g2) if g2 else (cref.msm_g1, ctx.msm_g1)
    want_lo = msm(pts[:n - 1], sc[:n - 1])
    want_hi = GM.oracle_plus(want_lo, pts[n - 1:], sc[n - 1:], g2)
    if k <= 12:
        assert np.array_equal(want_hi, msm(pts, sc))
    two_pass = (0, 1) if n >= GM.AUTO_16 else (0, 0)     # 2^20 - 1 pairs: c = 15, the one-pass sort; 2^20: c = 16, the two-pass sort
    for m, want, two in ((n - 1, want_lo, two_pass[0]), (n, want_hi, two_pass[1])):
        before = _sorts(ctx)
        got = run(pts[:m], sc[:m])
        assert np.array_equal(got, want), (k, m)
        assert _sorts(ctx) == (before[0] + 1 - two, before[1] + two), (k, m)


@pytest.mark.parametrize("k", range(7, 21))
def test_g1_on_both_sides_of_every_auto_c_step(ctx, k):
    """no knob: 2^k - 1 and 2^k WHIR-mix pairs with the edge scalars of both widths planted; at k = 20 the step to c = 16 is also the step
    from the one-pass to the two-pass sort, each counted once per MSM"""
    _auto_c_switch(ctx, k, False)


@pytest.mark.parametrize("k", range(7, 17))
def test_g2_on_both_sides_of_every_auto_c_step(ctx, k):
    _auto_c_switch(ctx, k, True)


# ---------------------------------------------------------------------------------------------------- d: the sort switch at c = 16
SWITCH_SIZES = (N18 - 1, N18, N18 + 1, N18 + 511, N18 + 513)


def _switch_wants(res, sizes):
    """the oracle's sum over the shortest prefix, extended pair by pair to the other sizes"""
    wants = {sizes[0]: res.oracle(sizes[0])}
    for a, b in zip(sizes, sizes[1:]):
        wants[b] = GM.oracle_plus(wants[a], res.pts[a:b], res.sc[a:b], res.g2)
    return wants


@pytest.fixture(scope="module")
def switch_g1(ctx):
    res = _Resident(ctx, *GM.case(SWITCH_SIZES[-1], [16], False, 6500, gen=_device_points(ctx)), False)
    yield res, _switch_wants(res, SWITCH_SIZES)
    res.free()


@pytest.fixture(scope="module")
def switch_g2(ctx):
    res = _Resident(ctx, *GM.case(SWITCH_SIZES[-1], [16], True, 6600, gen=_device_points(ctx)), True)
    yield res, _switch_wants(res, (N18, N18 + 513))
    res.free()


def _around_the_switch(ctx, res, wants, n):
    try:
        _width(ctx, 16)
        for one_pass in (0, 1):
            assert ctx.lib.mi_debug_set_msm_one_pass_sort(ctx.h, one_pass) == 0
            two = int(n >= N18 and not one_pass)          # below 2^18 the one-pass sort whatever the knob says
            for canonical in (False, True):
                before = _sorts(ctx)
                assert np.array_equal(res.msm(n, canonical), wants[n]), (n, one_pass, canonical)
                assert _sorts(ctx) == (before[0] + 1 - two, before[1] + two), (n, one_pass)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("n", SWITCH_SIZES)
def test_g1_around_the_sort_switch_at_c16(ctx, switch_g1, n):
    """c forced to 16: 2^18 - 1 pairs sort in one pass, 2^18 and more in two (one slice of 512 scalars more, one scalar short of and past
    it); from 2^18 on also the one-pass sort behind its knob; Montgomery and canonical scalars"""
    _around_the_switch(ctx, *switch_g1, n)


@pytest.mark.parametrize("n", [N18, N18 + 513])
def test_g2_around_the_sort_switch_at_c16(ctx, switch_g2, n):
    _around_the_switch(ctx, *switch_g2, n)


# ---------------------------------------------------------------------------------------------------- e: degenerate sets past the switch
@pytest.fixture(scope="module")
def sets18_g1(ctx):
    return GM.degenerate_sets(N18, 6700, gen=_device_points(ctx))


@pytest.fixture(scope="module")
def sets18_g2(ctx):
    return GM.degenerate_sets(N18, 6800, g2=True, gen=_device_points(ctx))


@pytest.fixture(scope="module")
def sets20_g1(ctx):
    return GM.degenerate_sets(GM.AUTO_16, 6900, gen=_device_points(ctx))


def _is_infinity_set(name):
    return name in ("zero", "all_infinity")


@pytest.mark.parametrize("name", GM.DEGENERATE)
def test_g1_degenerate_sets_at_c16_on_both_sorts(ctx, sets18_g1, name):
    """2^18 pairs, c = 16: the host side plans the item levels, the finisher and the grids from what the sort reports -- here a sort with no
    entry, with one, with every entry of a window in one key -- with the counted fullest bucket and with the worst-case bound"""
    pts, sc = sets18_g1[name]
    want = cref.msm_g1(pts, sc)
    assert GM.is_normalised_infinity(want) == _is_infinity_set(name)
    try:
        _width(ctx, 16)
        for one_pass in (0, 1):
            for bound in (0, 1):
                assert ctx.lib.mi_debug_set_msm_one_pass_sort(ctx.h, one_pass) == 0 and ctx.lib.mi_debug_set_msm_bound_levels(ctx.h, bound) == 0
                before = _sorts(ctx)
                assert np.array_equal(ctx.msm_g1(pts, sc), want), (name, one_pass, bound)      # (infinity: X = Y = 1, Z = 0, limb for limb)
                assert _sorts(ctx) == (before[0] + one_pass, before[1] + 1 - one_pass), (name, one_pass)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("name", ["zero", "one_value", "one_pair", "u128", "lone_last"])
def test_g2_degenerate_sets_at_c16_on_the_two_pass_sort(ctx, sets18_g2, name):
    pts, sc = sets18_g2[name]
    want = cref.msm_g2(pts, sc)
    assert GM.is_normalised_infinity(want) == _is_infinity_set(name)
    try:
        _width(ctx, 16)
        before = _sorts(ctx)
        assert np.array_equal(ctx.msm_g2(pts, sc), want), name
        assert _sorts(ctx) == (before[0], before[1] + 1)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("name", ["zero", "one_pair", "u128"])
def test_g1_degenerate_sets_at_2p20_as_a_caller_reaches_them(ctx, sets20_g1, name):
    """no knob at all: 2^20 pairs take c = 16 and the two-pass sort on their own"""
    pts, sc = sets20_g1[name]
    want = cref.msm_g1(pts, sc)
    before = _sorts(ctx)
    assert np.array_equal(ctx.msm_g1(pts, sc), want), name
    assert _sorts(ctx) == (before[0], before[1] + 1)
    assert GM.is_normalised_infinity(want) == _is_infinity_set(name)


# ---------------------------------------------------------------------------------------------------- f: degenerate sets, one-pass widths
@pytest.fixture(scope="module")
def sets3000():
    return GM.degenerate_sets(3000, 7000), GM.degenerate_sets(3000, 7100, g2=True)


@pytest.mark.parametrize("name", GM.DEGENERATE)
def test_g1_degenerate_sets_on_the_one_pass_widths(ctx, sets3000, name):
    pts, sc = sets3000[0][name]
    want = cref.msm_g1(pts, sc)
    try:
        for c in (3, 8, 13):
            _width(ctx, c)
            assert np.array_equal(ctx.msm_g1(pts, sc), want), (name, c)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("name", ["zero", "one_pair", "u128"])
def test_g2_degenerate_sets_at_c8(ctx, sets3000, name):
    pts, sc = sets3000[1][name]
    want = cref.msm_g2(pts, sc)
    try:
        _width(ctx, 8)
        assert np.array_equal(ctx.msm_g2(pts, sc), want), name
    finally:
        _reset(ctx)
