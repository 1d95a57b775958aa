"""Inputs shared by tests/test_ksum_cpu.py, tests/test_gpu_ksum.py and tests/test_gpu_verify_ksum.py: keys whose bases K[1..] are known
multiples of the generator (so the sum of a row is one integer and one scalar multiplication away), the rows of scalars that walk the
edges of the window tables, and the model of the window policy.  Nothing here calls the code under test."""
import os
import random
import subprocess
import numpy as np
import pyref as P
from helpers import fr_arr, g1_arr

HERE = os.path.dirname(os.path.abspath(__file__))
r = P.R_MOD
WIDTHS = (8, 4, 2)
SCALAR_BITS = 254
MIB = 1 << 20
DEFAULT_BUDGET = 64 * MIB
MAX_SLICES, TARGET_LANES, GRID_CAP_LANES = 1024, 1 << 18, 4096 * 64


def build_emu(so):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_ksum.cpp")])
    return so


# ---------------------------------------------------------------------------------------------------- the policy, written down again
def windows(c):
    return -(-SCALAR_BITS // c)


def table_bytes(ns, c):
    return ns * windows(c) * ((1 << c) - 1) * 64


def window_bits(ns, budget):
    return next((c for c in WIDTHS if ns and table_bytes(ns, c) <= budget), 0)


def budget_for(ns, c):
    """a budget under which a key of ns bases gets exactly the width c"""
    assert window_bits(ns, table_bytes(ns, c)) == c
    return table_bytes(ns, c)


def slices(ns, c, n):
    terms = ns * windows(c)
    return max(1, min(-(-TARGET_LANES // n), terms, MAX_SLICES))


# ---------------------------------------------------------------------------------------------------- keys in the exponent
KEY_KINDS = ("plain", "inf", "equal", "opposite")


def key_exps(ns, kind, seed=1):
    """e_j with K[1 + j] = e_j g.  inf: K[1] (and with ns > 2 the last base) at infinity; equal: K[2] = K[1]; opposite: K[2] = -K[1]"""
    rnd = random.Random(7000 + 10 * ns + seed)
    e = [rnd.randrange(1, r) for _ in range(ns)]
    if kind == "inf":
        e[0] = 0
        if ns > 2:
            e[-1] = 0
    elif kind == "equal" and ns > 1:
        e[1] = e[0]
    elif kind == "opposite" and ns > 1:
        e[1] = r - e[0]
    else:
        assert kind == "plain" or ns == 1
    return e


def sum_in_exponent(exps, row):
    return sum(s * e for s, e in zip(row, exps)) % r


def point(e):
    return P.g1_mul(P.G1_GEN, e % r) if e % r else None


def expected_points(exps, rows):
    """(n, 8): the sum of every row by ONE scalar multiplication of the generator"""
    return g1_arr([point(sum_in_exponent(exps, row)) for row in rows])


# ---------------------------------------------------------------------------------------------------- rows
TOP_WINDOW_ONLY = 0x2F << 248        # below r (its top byte is 0x30): only the partial 6-bit window of c = 8 is set


def edge_rows(ns, seed=3):
    """the rows the issue names, for any ns >= 1: all zero (infinity); all 1; all r - 1; only the top window set; byte values only;
    one non-zero scalar in the last column; full-width random; and with ns > 1 equal scalars in columns 0 and 1 (the doubling branch on a
    key with K[2] = K[1], cancellation with K[2] = -K[1]) and scalars of columns 0 and 1 that sum to r (cancellation with K[2] = K[1])"""
    rnd = random.Random(seed + ns)
    rows = [[0] * ns, [1] * ns, [r - 1] * ns, [TOP_WINDOW_ONLY] * ns, [rnd.randrange(256) for _ in range(ns)],
            [0] * (ns - 1) + [rnd.randrange(1, r)], [rnd.randrange(r) for _ in range(ns)]]
    if ns > 1:
        s = rnd.randrange(1, r)
        rows.append([s, s] + [0] * (ns - 2))
        rows.append([s, r - s] + [0] * (ns - 2))
        rows.append([s, s] + [rnd.randrange(r) for _ in range(ns - 2)])
    return rows


def batch_rows(ns, n, seed=5):
    """n rows: the edge rows first (as many as fit), then rows of mixed byte-valued and full-width scalars"""
    rnd = random.Random(100 * seed + ns + n)
    rows = edge_rows(ns, seed)[:n]
    while len(rows) < n:
        rows.append([rnd.randrange(256) if rnd.random() < 0.5 else rnd.randrange(r) for _ in range(ns)])
    return rows


def rows_arr(rows, ns):
    """-> (n, ns, 4) Montgomery words"""
    return fr_arr([s for row in rows for s in row]).reshape(len(rows), ns, 4)
