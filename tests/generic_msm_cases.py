"""Inputs shared by tests/test_generic_msm_cpu.py and tests/test_gpu_generic_msm.py: the generic Pippenger path (msm_sort_enqueue in
csrc/msm.hip: window widths 2..16, the one-pass counting sort and, at c = 16 from 2^18 pairs on, the two-pass sort with the window folded
into the key) at every width with the signed-digit edge scalars of that width, and the degenerate scalar sets whose sorts are empty, hold
one entry or pile every entry into one key.  The edge scalars are fixed_base_cases' own (edge_scalars, negative_digit_scalars: their
recipes take any width); what they reach at each width is asserted here with the pure-Python recoder FB.digits alone.  Nothing here calls
the code under test: only pyref's integers and the C oracle's generators and field operations (cref)."""
import random
import numpy as np
import pyref as P
import cref
from helpers import fr_arr, fp_arr, fp_vals, g1_pts, g2_pts
import fixed_base_cases as FB

r = P.R_MOD
WIDTHS = tuple(range(2, 17))
SORT_SWITCH = 1 << 18      # msm_sort_enqueue: c == 16 and n >= 2^18 (and 16 n < 2^31) take the two-pass sort
AUTO_16 = 1 << 20          # the first n at which auto_c (floor(log2 n) - 4, clamped to 3..16) gives 16
ONE_VALUE_WIDTHS = (5, 8, 16)   # the widths at which `one_value` is proven to have an entry in every window


def auto_c(n):
    """csrc/msm.hip auto_c in plain Python"""
    return min(16, max(3, n.bit_length() - 1 - 4))


def top_window(c):
    """the last window a scalar below r reaches: the one that holds bit 253"""
    return 253 // c


def straddling_windows(c):
    """the windows below the top one whose c bits lie in two 32-bit limbs"""
    return [w for w in range(top_window(c)) if (w * c) // 32 != (w * c + c - 1) // 32]


def assert_reaches_the_digit_edges(c, vals, every_window=True):
    """by FB.digits alone: vals hold a window-0 digit of -2^(c-1), a digit of 2^(c-1) - 1, a carry that enters the top window (whose own
    bits are zero) and a scalar whose every window below the top one is -2^(c-1); with every_window, also both extreme digits in every
    window that straddles a 32-bit limb at this width"""
    h, m = 1 << (c - 1), top_window(c)
    ds = [FB.digits(v, c) for v in vals]
    assert any(d[0] == -h for d in ds), c
    assert any(h - 1 in d for d in ds), c
    assert any((v >> (c * m)) == 0 and d[m] == 1 and d[m - 1] < 0 for v, d in zip(vals, ds)), c
    assert any(d[:m] == [-h] * m for d in ds), c
    for w in straddling_windows(c) if every_window else ():
        assert any(d[w] == -h for d in ds) and any(d[w] == h - 1 for d in ds), (c, w)
    assert all(len(d) == FB.nwin(c) and sum(x << (c * w) for w, x in enumerate(d)) == v for v, d in zip(vals, ds)), c


def _essential(c):
    """the few scalars that reach every edge assert_reaches_the_digit_edges names"""
    return FB.negative_digit_scalars(c) + FB.edge_scalars(c)[:2]


_WIDTH_SCALARS = {}


def width_scalars(c):
    """the edge scalars of width c: FB.edge_scalars(c) + FB.negative_digit_scalars(c) as they are, proven to reach the digit edges"""
    if c not in _WIDTH_SCALARS:
        vals = FB.edge_scalars(c) + FB.negative_digit_scalars(c)
        assert_reaches_the_digit_edges(c, vals)
        _WIDTH_SCALARS[c] = vals
    return list(_WIDTH_SCALARS[c])


def planted_scalars(c_list, room):
    """width_scalars of every width of c_list, in that order.  Where they do not fit into `room` places (n = 127 .. 256 with the widths 3
    and 4: 177 and 135 values), the essential ones of every width come first and the others follow in turn until the room is full: each
    width still reaches its four digit edges, which is asserted."""
    c_list = list(dict.fromkeys(c_list))
    full = [width_scalars(c) for c in c_list]
    if sum(map(len, full)) <= room:
        return sum(full, [])
    head = sum((_essential(c) for c in c_list), [])
    rest = [[v for v in f if v not in head] for f in full]
    tail = [f[i] for i in range(max(map(len, rest))) for f in rest if i < len(f)]
    vals = (head + tail)[:room]
    assert len(head) <= room
    for c in c_list:
        assert_reaches_the_digit_edges(c, vals, every_window=False)
    return vals


def _neg(row, g2):
    return FB._neg_g2(row) if g2 else FB._neg_g1(row)


def _points(n, seed, g2, gen):
    """n seeded points: the oracle's generator, or `gen(n, seed, g2)` (the GPU tests pass the device's, as the older large tests do: the
    oracle's takes 9 s for 2^18 G2 points).  Wherever they come from, the first ones are checked against the curve equation."""
    pts = np.ascontiguousarray((gen(n, seed, g2) if gen else (cref.gen_g2 if g2 else cref.gen_g1)(n, seed)), np.uint64)
    assert pts.shape == (n, 16 if g2 else 8)
    head = (g2_pts if g2 else g1_pts)(pts[:4])
    assert all(q is not None and (P.g2_is_on_curve if g2 else P.g1_is_on_curve)(q) for q in head) and len(set(head)) == len(head)
    return pts


def small_n(c):
    """the size of the small case of width c: 100 copies, the edge scalars, a ragged end -- no multiple of a wave (64) or a slice (512)"""
    n = 300 + len(width_scalars(c)) + 7
    assert n % 64 and n % 512
    return n


def case(n, c_list, g2, seed, dist=1, gen=None):
    """points and scalars (Montgomery) with what the older tests plant -- an infinity base, the scalars 0, 1 and r - 1, an equal pair and
    an opposite pair under equal scalars, 100 copies of one point under one scalar when n >= 300 -- and planted_scalars(c_list) from
    position 200 on (10 when n < 300).  Seeded WHIR-mix scalars (dist 1) fill the rest."""
    pts = _points(n, seed, g2, gen); sc = cref.gen_scalars(n, seed + 1, dist)
    assert n >= 20
    pts[3] = 0
    sc[1] = fr_arr([r - 1])[0]; sc[2] = 0; sc[4] = fr_arr([1])[0]
    pts[6] = pts[5]; sc[6] = sc[5]
    pts[8] = _neg(pts[7], g2); sc[8] = sc[7]
    pos = 10
    if n >= 300:
        pts[100:200] = pts[99]; sc[100:200] = sc[99]
        pos = 200
    vals = planted_scalars(c_list, n - pos)
    sc[pos:pos + len(vals)] = fr_arr(vals)
    return pts, sc


def planted_at(n):
    """where case() puts its edge scalars"""
    return 200 if n >= 300 else 10


def to_mont(canon):
    """(n, 4) canonical limbs -> Montgomery rows (the oracle's fe_to_mont)"""
    return cref.field_op(0, 4, np.ascontiguousarray(canon, np.uint64))


def jac_of(aff, g2):
    """an affine oracle point (all zero: infinity) as the normalised Jacobian point an MSM returns"""
    one = np.concatenate([fp_arr([1])[0], np.zeros(4, np.uint64)]) if g2 else fp_arr([1])[0]
    return np.concatenate([aff, one]) if aff.any() else np.concatenate([one, one, np.zeros_like(one)])


def oracle_plus(want, pts, sc, g2):
    """want + the MSM of a few more pairs: the oracle's MSM of those pairs and the oracle's point addition.  One large reference sum then
    serves every size that extends it by a handful of pairs."""
    w = 16 if g2 else 8
    msm, add = (cref.msm_g2, cref.g2_add) if g2 else (cref.msm_g1, cref.g1_add)
    aff = lambda j: (j[:w] if j[w:].any() else np.zeros(w, np.uint64)).reshape(1, w)
    return jac_of(add(aff(want), aff(msm(pts, sc)))[0], g2)


def _one_value(seed):
    """a full-width scalar whose every window up to the top one holds a non-zero digit at the widths ONE_VALUE_WIDTHS"""
    rnd = random.Random(seed)
    while True:
        v = rnd.randrange(1 << 253, r)
        if all(0 not in FB.digits(v, c)[:top_window(c) + 1] for c in ONE_VALUE_WIDTHS):
            return v


LONE_FIRST, LONE_LAST = 5, 1 << 240
ALL_MIN_16 = FB.edge_scalars(16)[0]                                   # 2^15 + sum_k (2^15 - 1) << 16 k, 1 <= k < 15
ALL_HALF_16 = sum((1 << 15) << (16 * k) for k in range(15))           # every 16-bit chunk 2^15
DEGENERATE = ("zero", "one", "r_minus_1", "one_value", "one_pair", "top_window", "u128", "all_min_digits_16", "all_half_chunks_16", "lone_first",
              "lone_last", "all_infinity")
assert FB.digits(ALL_MIN_16, 16) == [-(1 << 15)] * 15 + [1]
assert FB.digits(ALL_HALF_16, 16) == [-(1 << 15)] + [1 - (1 << 15)] * 14 + [1]
assert FB.digits(LONE_FIRST, 16) == [5] + [0] * 15 and FB.digits(LONE_LAST, 16) == [0] * 15 + [1]


def degenerate_sets(n, seed, g2=False, gen=None):
    """name -> (points, scalars), Montgomery scalars.  The sets share one array of seeded distinct points: nothing may write into it.
      zero, one, r_minus_1   every scalar that value
      one_value              one full-width value everywhere: every window has one key that holds n entries
      one_pair               the same value everywhere and one point everywhere: every addition at every level is a doubling
      top_window             k << 240 with seeded 1 <= k < 2^13: at c = 16 only the last window has entries
      u128                   seeded values below 2^128, with 2^128 - 1 and 2^127 at positions 0 and 1
      all_min_digits_16      every digit -2^15 at c = 16, the last carry alone in window 15: window 0 holds 2^15, the windows above it
                             2^15 - 1 and the carry
      all_half_chunks_16     sum_k 2^15 << 16 k, k < 15: the digit -2^15 in window 0, then -(2^15 - 1) in every window: the carries turn
                             the chunks 2^15 into the next bucket down
      lone_first, lone_last  a single non-zero scalar: 5 at index 0 (from c = 4 on one entry in the whole sort, in the first window) and
                             2^240 at index n - 1 (at c = 16 one entry, in the last window)
      all_infinity           seeded scalars, every base at infinity"""
    pts = _points(n, seed, g2, gen)
    seeded = cref.gen_scalars(n, seed + 1, 0)
    rng = np.random.default_rng(seed + 2)

    def every(v):
        return np.ascontiguousarray(np.tile(fr_arr([v]), (n, 1)))

    one_value = _one_value(seed + 3)
    same_pt = np.ascontiguousarray(np.tile(pts[:1], (n, 1)))
    top = np.zeros((n, 4), np.uint64)
    top[:, 3] = rng.integers(1, 1 << 13, n, dtype=np.uint64) << np.uint64(48)          # bit 240 = limb 3, bit 48
    u128 = np.zeros((n, 4), np.uint64)
    u128[:, :2] = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    u128[0] = cref.int_to_limbs((1 << 128) - 1); u128[1] = cref.int_to_limbs(1 << 127)
    first = np.zeros((n, 4), np.uint64); first[0] = fr_arr([LONE_FIRST])[0]
    last = np.zeros((n, 4), np.uint64); last[n - 1] = fr_arr([LONE_LAST])[0]
    sets = {"zero": (pts, np.zeros((n, 4), np.uint64)), "one": (pts, every(1)), "r_minus_1": (pts, every(r - 1)),
            "one_value": (pts, every(one_value)), "one_pair": (same_pt, every(one_value)), "top_window": (pts, to_mont(top)),
            "u128": (pts, to_mont(u128)), "all_min_digits_16": (pts, every(ALL_MIN_16)),
            "all_half_chunks_16": (pts, every(ALL_HALF_16)), "lone_first": (pts, first), "lone_last": (pts, last),
            "all_infinity": (np.zeros_like(pts), seeded)}
    assert tuple(sets) == DEGENERATE
    return sets


def is_normalised_infinity(jac):
    """the header's infinity of a normalised MSM result: X = Y = 1 (Montgomery), Z = 0; 12 limbs (G1) or 24 (G2: 1 = (1, 0))"""
    v = fp_vals(np.asarray(jac).reshape(-1, 4))
    return v == ([1, 1, 0] if len(v) == 3 else [1, 0, 1, 0, 0, 0])
