"""CPU suite: the inputs of tests/test_gpu_fixed_base_rprime.py are what that file says they are -- the edge scalars recode to the edge
digits at every window width 17..22 (a pure-Python recoder is the reference, the numpy recoder is checked against it), the skewed and flat
shapes satisfy their non-vacuity conditions from the inputs alone, the conversion's rows hold their special words, and the oracle takes
a twist point outside the r-torsion."""
import random
import numpy as np
import pytest
import pyref as P
import cref
from helpers import fr_arr, g2_arr, g2_from_jac
import bytes_cases as BC
import fixed_base_cases as FB

r = P.R_MOD


@pytest.mark.parametrize("c", FB.WIDTHS)
def test_edge_scalars_recode_to_the_edge_digits(c):
    h, m = 1 << (c - 1), 253 // c
    ev = FB.edge_scalars(c)
    assert FB.digits(ev[0], c)[:m] == [-h] * m and FB.digits(ev[0], c)[m] == 1      # every low digit -2^(c-1), the last carry alone above
    assert FB.digits(ev[1], c) == [h - 1] * m + [0] * (FB.nwin(c) - m)              # every digit the largest that needs no carry
    for k in range(1, m + 1):                                                       # all-ones chunks: -1, zeros that pass the carry on, then +1
        assert FB.digits((1 << (c * k)) - 1, c) == [-1] + [0] * (k - 1) + [1] + [0] * (FB.nwin(c) - k - 1)
        assert (1 << (c * k)) - 1 in ev
        d = FB.digits(1 << (c * k - 1), c)                                          # a lone top digit -2^(c-1)
        assert d[k - 1] == -h and d[k] == 1 and sum(map(abs, d)) == h + 1 and 1 << (c * k - 1) in ev
    assert (r - 1) // 2 in ev and r - 2 in ev
    rnd = random.Random(c)
    vals = ev + [0, 1, r - 1] + [rnd.randrange(r) for _ in range(200)]
    for v in vals:
        d = FB.digits(v, c)
        assert len(d) == FB.nwin(c) and all(-h <= x < h for x in d) and sum(x << (c * w) for w, x in enumerate(d)) == v
    # the numpy recoder (whole vectors, canonical limbs) gives the same digits
    got = FB.digits_np(FB.canonical(fr_arr(vals)), c)
    assert got.tolist() == [FB.digits(v, c) for v in vals]
    assert all(min(FB.digits(v, c)) < 0 for v in FB.negative_digit_scalars(c))


def test_planted_cases_hold_their_plants():
    for n, dist, c, _, _ in FB.G1_CASES:
        pts, sc = FB.g1_case(n, dist, c)
        assert pts.shape == (n, 8) and sc.shape == (n, 4)
        if n > 10:
            assert not pts[3].any() and not sc[2].any() and np.array_equal(pts[6], pts[5]) and np.array_equal(sc[8], sc[7])
            assert cref.g1_add(pts[7:8], pts[8:9])[0].any() == 0   # the opposite pair sums to infinity
        if n >= 300:
            assert (pts[100:200] == pts[99]).all() and np.array_equal(sc[200:202], fr_arr(FB.edge_scalars(c)[:2]))
    assert {c for _, _, c, _, _ in FB.G1_CASES} == set(FB.WIDTHS)
    assert {n for n, *_ in FB.G1_CASES} >= {63, 64, 65, FB.SLICE, FB.SLICE + 1, 2 * FB.SLICE + 1}


def test_skewed_shape_needs_three_item_levels():
    """non-vacuity of the skewed shape, from the inputs alone: the fullest bucket needs at least three accumulate passes at the plan's
    item sizes (16 then 8) and at a dense sort's 32"""
    _, sc, c = FB.skewed_shape()
    hist = FB.bucket_histogram(sc, c)
    assert hist.argmax() == 0 and hist[0] > 20000
    assert FB.item_levels(int(hist.max())) >= 3 and FB.item_levels(int(hist.max()), 32) >= 3
    assert FB.item_levels(1) == 1 and FB.item_levels(16) == 1 and FB.item_levels(17) == 2 and FB.item_levels(128) == 2 and FB.item_levels(129) == 3


@pytest.mark.parametrize("n", [FB.FLAT_N, FB.FLAT_N_RULE])
def test_flat_shapes_are_flat(n):
    """non-vacuity of the flat shapes: the fullest bucket holds at most twice the average (integer average, as msm_accum_enqueue forms
    it); the larger shape also reaches the average of 64 from which the automatic item size applies, and that size is not the plan's 16"""
    _, sc, c = FB.flat_shape(n)
    hist = FB.bucket_histogram(sc, c)
    avg = int(hist.sum()) // len(hist)
    assert len(hist) == 1 << (c - 1) and int(hist.max()) <= 2 * avg
    if n == FB.FLAT_N_RULE:
        assert avg >= 64
        t = avg
        while t > 32:
            t = -(-t // FB.ITEM_L2)
        assert 17 <= t <= 32


def test_conversion_rows_hold_the_special_words():
    p = P.Q_MOD
    for k in (2, 4):
        rows = FB.coord_rows(k, 260, 5)
        flat = {w for row in rows for w in row}
        q32 = -(-p // 32)
        assert {1, p - 1, (p - 1) // 2, (p + 1) // 2, q32, q32 - 1, P.fp_to_mont(1)} <= flat and rows[1] == [0] * k
        assert all(0 <= w < p for w in flat) and len(rows) == 260
        assert FB.limbs_to_words(FB.words_to_limbs(rows), k) == rows
        if k == 4:
            assert all(any(row.count(0) == 1 and row[z] == 0 for row in rows) for z in range(4))
    assert FB.times32([[q32 - 1, q32]]) == [[32 * (q32 - 1), 32 * q32 - p]]


def test_oracle_takes_a_twist_point_outside_the_r_torsion():
    """bytes_cases.twist_point_real_y: a twist point whose y has a zero imaginary part, not in the r-torsion.  The oracle's G2 MSM does
    plain curve arithmetic on canonical integer scalars, so it agrees with pyref's double-and-add on it"""
    Q = BC.twist_point_real_y()
    assert Q is not None and Q[1][1] == 0 and P.g2_is_on_curve(Q)
    assert P.g2_mul(Q, r) is not None
    for c in (17, 20):
        vals = FB.negative_digit_scalars(c) + [5]
        want = None
        for v in vals:
            want = P.g2_add(want, P.g2_mul(Q, v))
        got = cref.msm_g2(np.repeat(g2_arr([Q]), len(vals), axis=0), fr_arr(vals))
        assert g2_from_jac(got) == want
    for n, c in FB.G2_CASES:
        pts, sc = FB.g2_case(n, c, Q)
        assert pts.shape == (n, 16) and (pts == g2_arr([Q])[0]).all(axis=1).sum() == (1 if n == 1 else 5)
