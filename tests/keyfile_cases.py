"""Inputs and references shared by tests/test_keyfile_cpu.py and tests/test_gpu_keyfile.py: the compressed proving-key stream
(ProvingKey.WriteTo: oracle/pk_raw.py's layout field for field, every point through pyref.g1_compress / g2_compress), encoders of
single points in both encodings, and the list of twist points on which the two membership tests of the r-torsion are compared.
Nothing here calls the code under test."""
import functools
import os
import random
import struct
import subprocess
import numpy as np
import pyref as P
import cref
import pk_raw
import dlog_keys as D
import verify_cases as V
from helpers import fr_arr, g1_pts, g2_pts

HERE = os.path.dirname(os.path.abspath(__file__))
p, r = P.Q_MOD, P.R_MOD
RAW, COMPRESSED = 0, 1
NO_SUBGROUP_CHECK, SUBGROUP_BY_R = 1, 2
# the twist y^2 = x^3 + 3 / (9 + u) has r (2p - r) points; three of the cofactor's prime factors
COFACTOR = 2 * p - r
SMALL_PRIMES = (10069, 5864401, 1875725156269)


def build_emu(so):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_keyfile.cpp")])
    return so


def g1_enc(pt, encoding):
    return P.g1_compress(pt) if encoding == COMPRESSED else pk_raw.g1_raw(pt)


def g2_enc(pt, encoding):
    return P.g2_compress(pt) if encoding == COMPRESSED else pk_raw.g2_raw(pt)


def write_pk_stream(pk, commitment_keys=(), encoding=COMPRESSED):
    """pk_raw.write_pk_raw with every point in the given encoding (RAW: that writer itself)"""
    if encoding == RAW:
        return pk_raw.write_pk_raw(pk, commitment_keys)
    g1s = lambda pts: struct.pack(">I", len(pts)) + b"".join(P.g1_compress(q) for q in pts)
    g2s = lambda pts: struct.pack(">I", len(pts)) + b"".join(P.g2_compress(q) for q in pts)
    n = 1 << pk["log_n"]
    w = pow(P.FR_ROOT_2_28, 1 << (28 - pk["log_n"]), r)
    fr = lambda x: int(x % r).to_bytes(32, "big")
    out = [struct.pack(">Q", n), fr(pow(n, -1, r)), fr(w), fr(pow(w, -1, r)), fr(5), fr(pow(5, -1, r)), b"\x01"]
    out += [P.g1_compress(pk["alpha1"]), P.g1_compress(pk["beta1"]), P.g1_compress(pk["delta1"])]
    out += [g1s(pk["g1_a"]), g1s(pk["g1_b"]), g1s(pk["g1_z"]), g1s(pk["g1_k"])]
    out += [P.g2_compress(pk["beta2"]), P.g2_compress(pk["delta2"]), g2s(pk["g2_b"])]
    out += [struct.pack(">QQQ", pk["nb_wires"], sum(map(bool, pk["inf_a"])), sum(map(bool, pk["inf_b"])))]
    out += [pk_raw._bools(pk["inf_a"]), pk_raw._bools(pk["inf_b"]), struct.pack(">I", len(commitment_keys))]
    for basis, bes in commitment_keys:
        out += [g1s(basis), g1s(bes)]
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def toy(nc=200, npub=5, seed=31, n_ped=0):
    """tests/test_pk_raw.py's key: (constraint system, pyref key, domain, [(basis, basis_exp_sigma)]).  The key is pyref.toy_setup's:
    its exponents and its layout, with the point of every exponent from the oracle's batch scalar multiplication (oracle/groth16_ref.c)
    where toy_setup's own double-and-add in Python takes a quarter of a minute at nc = 1000.  Shared between tests: do not change it."""
    cs = P.ToyR1CS(nc, npub, seed); td = P.ToyTrapdoor(seed)
    g1, g2 = P.g1_mul, P.g2_mul
    P.g1_mul = P.g2_mul = lambda q, k: None
    try:
        pk, exps, dom = P.toy_setup(cs, td)
    finally:
        P.g1_mul, P.g2_mul = g1, g2
    sm1 = lambda sc: g1_pts(cref.batch_scalar_mul(D.G1, fr_arr(sc).reshape(-1, 4))) if len(sc) else []
    sm2 = lambda sc: g2_pts(cref.batch_scalar_mul(D.G2, fr_arr(sc).reshape(-1, 4), g2=True)) if len(sc) else []
    A, Bx, Kx, Z = (exps[k] for k in "ABKZ")
    nz_b = [x for x in Bx if x]
    pk.update(g1_a=sm1([x for x in A if x]), g1_b=sm1(nz_b), g2_b=sm2(nz_b), g1_k=sm1(Kx[cs.nb_public:]), g1_z=P.bit_reverse_perm(sm1(Z)))
    pk["alpha1"], pk["beta1"], pk["delta1"] = sm1([td.alpha, td.beta, td.delta])
    pk["beta2"], pk["delta2"] = sm2([td.beta, td.delta])
    keys = [(g1_pts(cref.gen_g1(7 + k, 40 + k)), g1_pts(cref.gen_g1(7 + k, 50 + k))) for k in range(n_ped)]
    return cs, pk, dom, keys


def twist_point(rnd):
    """a seeded point of the twist (of the whole group: its order is almost never a divisor of r)"""
    while True:
        x = (rnd.randrange(p), rnd.randrange(p))
        y = V.fp2_sqrt(P.fp2_add(P.fp2_mul(P.fp2_sqr(x), x), P.G2_B))
        if y is not None:
            return (x, y)


def subgroup_cases(seed=11):
    """[(name, point of the twist, in the r-torsion by [r] Q in Python)]: 29 points, both verdicts among them"""
    rnd = random.Random(seed)
    n = r * COFACTOR
    assert all(COFACTOR % q == 0 for q in SMALL_PRIMES)
    pts = [("generator", P.G2_GEN), ("multiple of the generator", P.g2_mul(P.G2_GEN, rnd.randrange(1, r)))]
    ts = [twist_point(rnd) for _ in range(3)]
    pts += [(f"twist point {i}", t) for i, t in enumerate(ts)]
    pts += [(f"cofactor x twist point {i}", P.g2_mul(t, COFACTOR)) for i, t in enumerate(ts)]
    small = [(f"order-{q} part of twist point {i}", P.g2_mul(t, n // q)) for i, t in enumerate(ts) for q in SMALL_PRIMES]
    pts += small
    pts += [(name + " + generator", P.g2_add(c, P.G2_GEN)) for name, c in small]
    rest = r * SMALL_PRIMES[0] * SMALL_PRIMES[1] * SMALL_PRIMES[2]
    pts += [(f"twist point {i} x r x the three primes", P.g2_mul(t, rest)) for i, t in enumerate(ts)]
    out = [(name, q, P.g2_mul(q, r) is None) for name, q in pts]
    assert len(out) == 29 and all(q is not None and P.g2_is_on_curve(q) for _, q, _ in out)
    assert {v for _, _, v in out} == {True, False}
    return out


def codec_points(n, seed, g2=False):
    """n points for the bulk codecs: multiples of the generator of both signs, infinities, and (G2) a point with y.A1 = 0"""
    import bytes_cases as BC
    rnd = random.Random(seed)
    gen, mul, neg = (P.G2_GEN, P.g2_mul, P.g2_neg) if g2 else (P.G1_GEN, P.g1_mul, P.g1_neg)
    base = [mul(gen, rnd.randrange(1, 1 << 30)) for _ in range(min(n, 12))]
    base += [neg(q) for q in base]
    if g2:
        real_y = BC.twist_point_real_y(64)
        base += [real_y, P.g2_neg(real_y)]
    out = [None if rnd.randrange(9) == 0 else base[rnd.randrange(len(base))] for _ in range(n)]
    return out
