"""CPU suite: the per-lane text of the phase-2 kernels (include/mi355x_groth16_phase2.h) on the host.  tests/cpp/phase2_host.cpp, its own
main, built with -fsanitize=address,undefined by `make sanitize-phase2`, runs the butterfly and the stage of the point NTT
(csrc/point_ntt.cuh) and the term and the run of a sparse sum of points (csrc/sparse_points.cuh) -- the text phase2.hip's kernels run --
for G1 and G2; what it prints is compared here with oracle/pyref.py: double-and-add over exponents computed in Python integers.  No
library is preloaded anywhere."""
import os
import subprocess
import pytest
import pyref as P
from gpu_common import ROOT

R = P.R_MOD
TAU = 0x1F3A9C5D7E2B4681_0FEDCBA987654321_1122334455667788 % R
FULL = 0x2A3C09F0A58A7E85_00E0A7EB8EF62ABC_402D111E41112ED4_9BD61B6E725B19F1 % R
# every path a scalar can take: nothing, an addition, a subtraction, xyzz_mul_u32 on c or on r - c, the full double-and-add
COEFFS = [1, R - 1, 2, R - 2, (1 << 32) - 1, 1 << 32, R - (1 << 32), R - (1 << 32) + 1, FULL, 0]


def tau_2n_root(log_n):
    """a primitive 2N-th root of unity: tau^N = -1"""
    t = pow(P.FR_ROOT_2_28, 1 << (P.FR_TWO_ADICITY - log_n - 1), R)
    assert pow(t, 1 << log_n, R) == R - 1
    return t


def lagrange(log_n, tau):
    """L_i(tau), i < N, by the definition sum_k w^(-i k) tau^k / N (defined for tau on the 2N-th roots too, where tau^N = -1)"""
    n = 1 << log_n
    w_inv = P.fr_inv(P.Domain(n).gen) if n > 1 else 1
    n_inv = P.fr_inv(n)
    return [sum(pow(w_inv, i * k, R) * pow(tau, k, R) for k in range(n)) * n_inv % R for i in range(n)]


def _mul(group, k):
    k %= R
    if group == 1:
        return None if k == 0 else P.g1_mul(P.G1_GEN, k)
    return None if k == 0 else P.g2_mul(P.G2_GEN, k)


def _parse(group, line):
    if line == "inf":
        return None
    v = [int(x, 16) for x in line.split()]
    return (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))


def _cases():
    """[(command line, group, the exponents of the points it must print)]"""
    out = []
    for group in (1, 2):
        for log_n in (0, 1, 2, 3, 4):
            out.append((f"ntt {group} {log_n} {TAU:x}", group, lagrange(log_n, TAU)))
        for log_n in (1, 3, 4):   # tau^N = -1
            t = tau_2n_root(log_n)
            out.append((f"ntt {group} {log_n} {t:x}", group, lagrange(log_n, t)))
        # one butterfly on equal, opposite and absent operands, with every kind of factor
        for ea, eb in ((7, 7), (7, R - 7), (0, 9), (9, 0), (0, 0), (11, 5)):
            for kt, kb in ((1, 1), (R - 1, 3), (FULL, R - 1), (5, FULL)):
                out.append((f"bfly {group} {ea:x} {eb:x} {kt:x} {kb:x}", group, [kt * (ea + eb), kb * (ea - eb)]))
        for log_n, tau in ((3, TAU), (3, tau_2n_root(3))):
            L = lagrange(log_n, tau)
            cols = {
                "every coefficient path": [(i % 8, c) for i, c in enumerate(COEFFS)],
                "c and r - c on one row: the sum passes through infinity": [(2, FULL), (2, R - FULL), (5, 3)],
                "a column that cancels to zero": [(1, 6), (1, R - 4), (1, R - 2)],
                "coefficient 0 alone": [(4, 0)],
                "duplicates: the same row twice, so a doubling": [(6, 1), (6, 1), (6, FULL), (6, FULL)],
                "an empty column": [],
            }
            for entries in cols.values():
                line = f"col {group} {log_n} {tau:x} {len(entries)}" + "".join(f" {r:x} {c:x}" for r, c in entries)
                out.append((line, group, [sum(c * L[r] for r, c in entries)]))
    return out


def test_the_lagrange_definitions_agree():
    """this file's L_i against pyref.lagrange_at's closed form, where that is defined (tau off the domain)"""
    for log_n in (1, 2, 4):
        assert lagrange(log_n, TAU) == P.lagrange_at(P.Domain(1 << log_n), TAU)


def test_phase2_lane_bodies_on_the_host():
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-phase2"])
    cases = _cases()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "phase2_host_asan")], input="".join(c[0] + "\n" for c in cases), capture_output=True, text=True,
                         env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    lines = res.stdout.splitlines()
    at = 0
    known = {}
    for cmd, group, exps in cases:
        assert lines[at] == cmd
        got = [_parse(group, l) for l in lines[at + 1:at + 1 + len(exps)]]
        at += 1 + len(exps)
        want = [known.setdefault((group, e % R), _mul(group, e)) for e in exps]
        assert got == want, cmd
    assert at == len(lines)
    # the cancelling column and the tau^N = -1 transforms were among them
    assert any(c[0].startswith("col") and c[2][0] % R == 0 and len(c[0].split()) > 5 for c in cases)
