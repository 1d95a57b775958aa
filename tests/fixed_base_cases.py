"""Inputs shared by tests/test_fixed_base_cases_cpu.py and tests/test_gpu_fixed_base_rprime.py: coordinate words for the table
conversion (mi_msm_table_to_rprime_*: every 256-bit word times 2^5 mod p), the signed-digit recoding of the fixed-base sort in plain
Python (csrc/msm2_core.cuh Msm2Digits: digits in [-2^(c-1), 2^(c-1) - 1], the carry chained from window 0) and in numpy for whole
scalar vectors, bucket histograms and item-level counts from them, and the MSM cases with their planted points and scalars.  Nothing
here calls the code under test: only pyref's integers and the C oracle's generators (cref)."""
import random
import numpy as np
import pyref as P
import cref
from helpers import fr_arr, g1_arr, g1_pts, g2_arr, g2_pts

p, r = P.Q_MOD, P.R_MOD
WIDTHS = (17, 18, 19, 20, 21, 22)
SLICE = 512            # MSM2_SLICE: scalars per pass-1 workgroup of the fixed-base sort
ITEM_L1, ITEM_L2 = 16, 8   # the plan's item sizes (msm_accum_enqueue); a dense sort's level 1 takes 32


# ---------------------------------------------------------------------------------------------------- the conversion's words
def words_to_limbs(rows):
    """rows of 256-bit integers -> (n, 4 * len(row)) uint64, little-endian limbs"""
    return np.array([sum((cref.int_to_limbs(w) for w in row), []) for row in rows], dtype=np.uint64)


def limbs_to_words(arr, k):
    """(n, 4k) uint64 -> rows of k integers"""
    return [[cref.limbs_to_int(row[4 * j:4 * j + 4]) for j in range(k)] for row in np.asarray(arr).reshape(-1, 4 * k)]


def times32(rows):
    return [[(w * 32) % p for w in row] for row in rows]


def coord_rows(k, n_rows, seed):
    """n_rows rows of k words below p (k = 2: G1 x, y; k = 4: G2 x.a0, x.a1, y.a0, y.a1).  Row 0 is a wrapping row (what n_points = 1
    converts), row 1 all zero (the infinity marker); then the doubling wraps on both sides, the first and last value whose five
    doublings do not wrap, the Montgomery one, for k = 4 the rows with exactly one zero component; seeded values below p fill the rest."""
    rnd = random.Random(seed)
    q32 = -(-p // 32)   # ceil(p / 32): 32 * q32 >= p wraps, 32 * (q32 - 1) < p does not
    mont_one = P.fp_to_mont(1)
    special = [1, p - 1, (p - 1) // 2, (p + 1) // 2, q32, q32 - 1, mont_one, p - 2, 2, q32 + 1, (p - 1) // 32, p // 2 + 2]
    assert 32 * (q32 - 1) < p <= 32 * q32
    rows = [[p - 1 - j for j in range(k)], [0] * k]
    for i in range(0, len(special), k):
        rows.append((special[i:i + k] + special[:k])[:k])
    rows.append(list(reversed(special[:k])))
    if k == 4:
        for z in range(4):
            row = [rnd.randrange(1, p) for _ in range(4)]
            row[z] = 0
            rows.append(row)
            row = [p - 1, (p + 1) // 2, q32, mont_one]
            row[z] = 0
            rows.append(row)
    while len(rows) < n_rows:
        rows.append([rnd.randrange(p) for _ in range(k)])
    return rows[:n_rows]


# ---------------------------------------------------------------------------------------------------- signed digits
def nwin(c):
    return (256 + c - 1) // c


def digits(v, c):
    """the signed c-bit digits of the canonical scalar v, window 0 first (the pure-Python reference of the recoding)"""
    out, carry = [], 0
    for w in range(nwin(c)):
        d = ((v >> (w * c)) & ((1 << c) - 1)) + carry
        carry = int(d >= 1 << (c - 1))
        out.append(d - (carry << c))
    assert carry == 0
    return out


def digits_np(canon, c):
    """the same for (n, 4) uint64 canonical limbs -> (n, nwin) int64"""
    canon = np.ascontiguousarray(canon, np.uint64)
    n = canon.shape[0]
    out = np.zeros((n, nwin(c)), np.int64)
    carry = np.zeros(n, np.int64)
    mask = np.uint64((1 << c) - 1)
    for w in range(nwin(c)):
        bit = w * c
        limb, sh = bit >> 6, bit & 63
        raw = canon[:, limb] >> np.uint64(sh)
        if sh + c > 64 and limb + 1 < 4:
            raw = raw | (canon[:, limb + 1] << np.uint64(64 - sh))
        d = (raw & mask).astype(np.int64) + carry
        carry = (d >= (1 << (c - 1))).astype(np.int64)
        out[:, w] = d - (carry << c)
    assert not carry.any()
    return out


def canonical(sc_mont):
    """Montgomery Fr rows -> canonical limbs (the oracle's fe_from_mont)"""
    return cref.field_op(0, 5, sc_mont)


def bucket_histogram(sc_mont, c):
    """entries per bucket of the fixed-base sort of these scalars: bucket |d| - 1 for every non-zero digit d, one bucket set of 2^(c-1)"""
    d = digits_np(canonical(sc_mont), c)
    keys = np.abs(d[d != 0]) - 1
    return np.bincount(keys, minlength=1 << (c - 1))


def item_levels(fullest, l1=ITEM_L1, l2=ITEM_L2):
    """accumulate passes the item machinery needs for a bucket of `fullest` entries (run_levels: ceil(m / L) partial sums go on while
    more than one is left)"""
    levels, m, L = 1, fullest, l1
    while -(-m // L) > 1:
        m = -(-m // L); L = l2; levels += 1
    return levels


def edge_scalars(c):
    """scalars at the edges of the signed c-bit digits, after the recipe of dlog_keys.edge_values for ONE width (21 included).  The
    first two are the all-low-digits -2^(c-1) and the all 2^(c-1) - 1 values; then the all-ones chunks 2^(ck) - 1, a lone top digit
    -2^(c-1) for every k, every chunk 2^(c-1), (r - 1) / 2 and r - 2."""
    h = 1 << (c - 1)
    m = 253 // c                                                      # whole windows below r
    vals = [h + sum((h - 1) << (c * k) for k in range(1, m)), sum((h - 1) << (c * k) for k in range(m))]
    vals += [(1 << (c * k)) - 1 for k in range(1, m + 1)]
    vals += [1 << (c * k - 1) for k in range(1, m + 1)]
    vals += [sum(h << (c * k) for k in range(m)), (r - 1) // 2, r - 2]
    assert all(0 < v < r for v in vals)
    return vals


# ---------------------------------------------------------------------------------------------------- MSM cases
G1_CASES_OLD = [(1, 0, 17, 0, 0), (300, 1, 17, 64, 6), (5000, 0, 18, 1000, 15), (70000, 1, 20, 0, 0), (200000, 0, 22, 0, 9),
                (513, 1, 19, 100, 12), (66000, 0, 21, 4096, 10)]      # test_fixed_base_msm_g1_vs_oracle's
G1_CASES = G1_CASES_OLD + [(63, 1, 21, 0, 0), (64, 0, 21, 0, 0), (65, 1, 22, 0, 0),            # width 21 and the wave edges
                           (512, 0, 17, 0, 0), (513, 1, 21, 100, 12), (1025, 0, 19, 64, 6),     # the slice of 512 scalars and one more
                           (70000, 1, 21, 0, 0)]
G1_KNOB_CASES = [(300, 1, 17, 64, 6), (5000, 0, 18, 1000, 15), (70000, 1, 21, 0, 0)]
G2_CASES = [(n, c) for n in (1, 65, 3000) for c in (17, 18, 20)]


def _neg_g1(row):
    return g1_arr([P.g1_neg(g1_pts(row.reshape(1, 8))[0])])[0]


def _neg_g2(row):
    return g2_arr([P.g2_neg(g2_pts(row.reshape(1, 16))[0])])[0]


def g1_case(n, dist, c):
    """points and scalars of a G1 case with what the older tests plant (n > 10: an infinity base, scalars 0, 1 and r - 1, a repeated
    pair and an opposite pair with equal scalars; n >= 300: 100 copies of one point with one scalar, the edge scalars of width c)"""
    pts = cref.gen_g1(n, 1300 + n + 7 * c); sc = cref.gen_scalars(n, 1400 + n + 7 * c, dist)
    if n > 10:
        pts[3] = 0
        sc[1] = fr_arr([r - 1])[0]; sc[2] = 0; sc[4] = fr_arr([1])[0]
        pts[6] = pts[5]; sc[6] = sc[5]
        pts[8] = _neg_g1(pts[7]); sc[8] = sc[7]
    if n >= 300:
        pts[100:200] = pts[99]; sc[100:200] = sc[99]
        ev = edge_scalars(c)
        assert 200 + len(ev) <= n
        sc[200:200 + len(ev)] = fr_arr(ev)
    return pts, sc


def negative_digit_scalars(c):
    """scalars whose digits at width c are negative: a lone -2^(c-1), a -1 with its carry, every low digit -2^(c-1), r - 1"""
    out = [1 << (c - 1), (1 << c) - 1, edge_scalars(c)[0], r - 1]
    assert all(min(digits(v, c)) < 0 for v in out)
    return out


def g2_case(n, c, real_y):
    """a G2 case: the repeated and opposite triples of test_msm_g2_repeated_and_opposite_points, an infinity base, and `real_y` (a
    twist point whose y has a zero imaginary part, bytes_cases.twist_point_real_y) under scalars with negative digits and one positive.
    n = 1 is that point alone under the all-low-digits -2^(c-1) scalar."""
    pts = cref.gen_g2(n, 321 + n + c); sc = cref.gen_scalars(n, 322 + n + c, 1)
    q = g2_arr([real_y])[0]
    if n == 1:
        pts[0] = q; sc[0] = fr_arr([edge_scalars(c)[0]])[0]
        return pts, sc
    for i in range(0, min(60, n - 8), 3):
        pts[i + 1] = pts[i]; sc[i + 1] = sc[i]
        pts[i + 2] = _neg_g2(pts[i]); sc[i + 2] = sc[i]
    neg = negative_digit_scalars(c)
    k = n - len(neg) - 2
    pts[k:k + len(neg) + 1] = q
    sc[k:k + len(neg)] = fr_arr(neg); sc[k + len(neg)] = fr_arr([5])[0]
    pts[n - 1] = 0
    return pts, sc


def g2_generic_case(n, seed, real_y):
    """a generic G2 MSM with `real_y` planted under scalars whose digits are negative at every generic window width (8..16)"""
    pts = cref.gen_g2(n, seed); sc = cref.gen_scalars(n, seed + 1, 1)
    vals = [5, r - 1, r - 2]
    for c in range(8, 17):
        vals += [1 << (c - 1), (1 << c) - 1, sum((1 << (c - 1)) << (c * k) for k in range(253 // c))]
    assert len(vals) + 20 <= n
    pts[10:10 + len(vals)] = g2_arr([real_y])[0]
    sc[10:10 + len(vals)] = fr_arr(vals)
    pts[3] = 0
    return pts, sc


def skewed_shape():
    """n = 70000, c = 17, WHIR-mix scalars with every third equal to 1: bucket 0 holds more than 20000 entries"""
    n, c = 70000, 17
    pts = cref.gen_g1(n, 8100); sc = cref.gen_scalars(n, 8101, 1)
    sc[::3] = fr_arr([1])[0]
    return pts, sc, c


def flat_shape(n):
    """c = 17, uniform scalars: 15 entries per scalar spread evenly over 2^16 buckets (2^17 distinct points, repeated beyond that: the
    repeats meet under independent scalars)"""
    pts = cref.gen_g1(min(n, 1 << 17), 8200); sc = cref.gen_scalars(n, 8201 + (n >> 16), 0)
    if n > pts.shape[0]:
        pts = np.ascontiguousarray(np.tile(pts, (-(-n // pts.shape[0]), 1))[:n])
    return pts, sc, 17


FLAT_N = 1 << 17          # the issue's flat shape: about 30 entries a bucket
FLAT_N_RULE = 9 << 16     # 134 entries a bucket: msm_accum_enqueue's rule also asks for an average of at least 64, and chooses a size of its
                          # own only where average / 8^k falls into 17..32 (here 17)
