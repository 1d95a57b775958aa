"""CPU suite for the generic Pippenger path: the inputs of tests/test_gpu_generic_msm.py are what generic_msm_cases says they are (by the
pure-Python recoder alone), and the per-thread bodies of csrc/msm_core.cuh (one-pass sort) and csrc/msm2_core.cuh with the window folded
into the key (two-pass sort; at c = 16 the compile-time Msm2Digits::at<16> through MSM2_FOR_C) give the oracle's sum on them at every
window width 2..16 and on every degenerate scalar set -- the host build of tests/emu/emu.cpp, as test_device_headers_on_host.py builds it."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pyref as P
import cref
from helpers import fr_arr, fr_vals, g1_pts
import fixed_base_cases as FB
import generic_msm_cases as GM

HERE = os.path.dirname(os.path.abspath(__file__))
r = P.R_MOD


@pytest.fixture(scope="module")
def emu():
    """tests/emu/libemu.so as test_device_headers_on_host.py builds it; built again only when a source it includes is newer"""
    so = os.path.join(HERE, "emu", "libemu.so")
    src = os.path.join(HERE, "emu", "emu.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "gnark-whir_amd", "csrc")
    deps = [src] + [os.path.join(d, f) for d in (csrc, os.path.dirname(src)) for f in os.listdir(d) if f.endswith((".cuh", ".h", ".hpp"))]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(out, want):
    """the emu's affine sum against the oracle's normalised Jacobian one (infinity: all zero against Z = 0)"""
    return np.array_equal(out, want[:8]) if want[8:].any() else not out.any()


def _both_sorts(emu, pts, sc, c, mont=1):
    """the one-pass bodies and the two-pass bodies with wkeys = 1, with the arguments the issue lists"""
    n = pts.shape[0]
    pts, sc = np.ascontiguousarray(pts), np.ascontiguousarray(sc)
    one, two = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    assert emu.emu_msm_g1(_p(one), _p(pts), _p(sc), n, mont, c, 2, 4, 4, 7) >= 1
    gbits = 1 if c == 2 else min(c - 1, 6)
    assert emu.emu_msm2_g1(_p(two), _p(pts), _p(sc), n, mont, c, 2, 16, 4, 4, 5, gbits, 1) >= 0   # chunks of the second pass: 0 for an empty sort
    return one, two


# ---------------------------------------------------------------------------------------------------- the cases themselves
@pytest.mark.parametrize("c", GM.WIDTHS)
def test_width_scalars_reach_the_digit_edges(c):
    """width_scalars(c) is FB.edge_scalars + FB.negative_digit_scalars unchanged, every value has digits at this width, and the set holds
    the edges the GPU tests rely on (asserted inside width_scalars; spelled out once more here on the named values)"""
    h, m = 1 << (c - 1), GM.top_window(c)
    vals = GM.width_scalars(c)
    assert vals == FB.edge_scalars(c) + FB.negative_digit_scalars(c) and all(0 < v < r for v in vals)
    GM.assert_reaches_the_digit_edges(c, vals)
    assert FB.digits(1 << (c - 1), c)[:2] == [-h, 1]                                  # a window-0 digit of -2^(c-1)
    assert FB.digits(vals[1], c)[:m] == [h - 1] * m                                   # every digit the largest that needs no carry
    d = FB.digits(vals[0], c)
    assert d[:m] == [-h] * m and d[m] == 1 and vals[0] >> (c * m) == 0                # every low window -2^(c-1), the carry alone on top
    assert m == FB.nwin(c) - 1 or not any(d[m + 1:])
    if 32 % c:
        assert GM.straddling_windows(c)
    # a carry that runs through every window: 2^(c m) - 1 is -1, zeros that pass the carry on, then +1 in the top window
    assert (1 << (c * m)) - 1 in vals and FB.digits((1 << (c * m)) - 1, c)[:m + 1] == [-1] + [0] * (m - 1) + [1]


def test_every_width_fits_the_shared_vectors():
    """the 1329 edge scalars of all fifteen widths fit the G2 case of 2^14 + 37 pairs; the small cases cut down for n < 257 keep the edges"""
    assert sum(len(GM.width_scalars(c)) for c in GM.WIDTHS) == 1329
    pts, sc = GM.case((1 << 14) + 37, GM.WIDTHS, True, 1)
    got = fr_vals(sc[200:200 + 1329])
    assert got == sum((GM.width_scalars(c) for c in GM.WIDTHS), [])
    assert not pts[3].any() and not sc[2].any() and fr_vals(sc[1:2]) == [r - 1] and fr_vals(sc[4:5]) == [1]
    assert np.array_equal(pts[6], pts[5]) and np.array_equal(sc[8], sc[7]) and not cref.g2_add(pts[7:8], pts[8:9])[0].any()
    assert (pts[100:200] == pts[99]).all() and (sc[100:200] == sc[99]).all()
    for n in (127, 128, 255, 256):
        cs = sorted({GM.auto_c(n), GM.auto_c(n + 1), 3})
        vals = GM.planted_scalars(cs, n - 10)
        assert len(vals) == n - 10
        for c in cs:
            GM.assert_reaches_the_digit_edges(c, vals, every_window=False)
    assert [GM.auto_c(n) for n in (1, 127, 128, 255, 256, (1 << 20) - 1, 1 << 20, 1 << 27)] == [3, 3, 3, 3, 4, 15, 16, 16]


def test_degenerate_sets_are_what_they_say():
    n = 700
    sets = GM.degenerate_sets(n, 5)
    assert tuple(sets) == GM.DEGENERATE
    pts = sets["zero"][0]
    assert len({row.tobytes() for row in pts}) == n and all(p_ is not None for p_ in g1_pts(pts[:50]))
    val = {k: fr_vals(v[1]) for k, v in sets.items()}
    assert val["zero"] == [0] * n and val["one"] == [1] * n and val["r_minus_1"] == [r - 1] * n
    v = val["one_value"][0]
    assert val["one_value"] == [v] * n and val["one_pair"] == [v] * n and v >> 253
    for c in GM.ONE_VALUE_WIDTHS:
        assert 0 not in FB.digits(v, c)[:GM.top_window(c) + 1]
    assert (sets["one_pair"][0] == pts[0]).all()
    assert all(x % (1 << 240) == 0 and 1 <= x >> 240 < 1 << 13 for x in val["top_window"]) and len(set(val["top_window"])) > n // 2
    assert all(FB.digits(x, 16)[:15] == [0] * 15 for x in val["top_window"][:20])
    assert all(x < 1 << 128 for x in val["u128"]) and val["u128"][:2] == [(1 << 128) - 1, 1 << 127] and len(set(val["u128"])) == n
    assert val["all_min_digits_16"] == [GM.ALL_MIN_16] * n and val["all_half_chunks_16"] == [GM.ALL_HALF_16] * n
    assert GM.ALL_HALF_16 == sum((1 << 15) << (16 * k) for k in range(15)) and FB.digits(GM.ALL_MIN_16, 16)[:15] == [-(1 << 15)] * 15
    assert val["lone_first"] == [GM.LONE_FIRST] + [0] * (n - 1) and val["lone_last"] == [0] * (n - 1) + [GM.LONE_LAST]
    assert not sets["all_infinity"][0].any() and len(set(val["all_infinity"])) == n
    assert GM.is_normalised_infinity(cref.msm_g1(*sets["zero"])) and GM.is_normalised_infinity(cref.msm_g1(*sets["all_infinity"]))
    s2 = GM.degenerate_sets(40, 6, g2=True)
    assert s2["one"][0].shape == (40, 16) and GM.is_normalised_infinity(cref.msm_g2(*s2["zero"]))
    assert np.array_equal(GM.to_mont(np.array([cref.int_to_limbs(7), cref.int_to_limbs(r - 1)], np.uint64)), fr_arr([7, r - 1]))
    assert np.array_equal(FB.canonical(GM.to_mont(FB.canonical(sets["u128"][1]))), FB.canonical(sets["u128"][1]))


def test_oracle_plus_extends_a_reference_sum():
    """the GPU tests take one large oracle sum per vector and extend it by the last few pairs: that sum equals the oracle's own over the
    longer prefix, on both curves, with the infinity cases on every side"""
    for g2, msm in ((False, cref.msm_g1), (True, cref.msm_g2)):
        pts, sc = GM.case(120, [16], g2, 70 + g2)
        for lo, hi in ((100, 101), (100, 120), (0, 1), (7, 9), (2, 3)):     # (7, 9): adds the opposite pair; (2, 3): scalar 0 plus an infinity base
            assert np.array_equal(GM.oracle_plus(msm(pts[:lo], sc[:lo]), pts[lo:hi], sc[lo:hi], g2), msm(pts[:hi], sc[:hi])), (g2, lo, hi)
        inf = msm(pts[:0], sc[:0])
        assert GM.is_normalised_infinity(inf) and GM.is_normalised_infinity(GM.oracle_plus(inf, pts[2:4], sc[2:4], g2))
    assert [GM.small_n(c) % 64 != 0 for c in GM.WIDTHS] == [True] * 15


# ---------------------------------------------------------------------------------------------------- the per-thread bodies on the host
@pytest.mark.parametrize("c", GM.WIDTHS)
def test_edge_scalars_through_both_sorts_match_oracle(emu, c):
    """every width, the one-pass and the two-pass bodies, Montgomery and canonical scalars, on the edge scalars of that width with an
    infinity base, 0, 1, r - 1, an equal and an opposite pair"""
    n = len(GM.width_scalars(c)) + 20
    pts, sc = GM.case(n, [c], False, 4000 + c)
    assert fr_vals(sc[10:n - 10]) == GM.width_scalars(c)
    want = cref.msm_g1(pts, sc)
    assert want[8:].any()
    canon = FB.canonical(sc)
    for mont, s in ((1, sc), (0, canon)):
        one, two = _both_sorts(emu, pts, s, c, mont)
        assert _same(one, want), (c, mont, "one-pass")
        assert _same(two, want), (c, mont, "two-pass")


@pytest.fixture(scope="module")
def sets700():
    return GM.degenerate_sets(700, 4100)


@pytest.mark.parametrize("name", GM.DEGENERATE)
def test_degenerate_sets_through_both_sorts_match_oracle(emu, sets700, name):
    """an empty sort, one entry, every entry in one key of every window, 128-bit scalars: both sorts' bodies at c = 5 and c = 16"""
    pts, sc = sets700[name]
    want = cref.msm_g1(pts, sc)
    assert bool(want[8:].any()) == (name not in ("zero", "all_infinity"))
    for c in (5, 16):
        one, two = _both_sorts(emu, pts, sc, c)
        assert _same(one, want), (name, c, "one-pass")
        assert _same(two, want), (name, c, "two-pass")
