"""Inputs and references shared by tests/test_decode_cpu.py and tests/test_gpu_verify_bytes.py: the Python references of what reads a
proof's bytes (hashlib's SHA-256, a ten-line expand_message_xmd, the BSB22 hashes as go/mi355x/verify.go states them, square roots by
pow), the edge lists of the decoders, and forged proofs (tests/verify_forge.py) whose commitment values and fold challenge ARE those
hashes -- with every discrete log known, a proof that must be accepted exists for whatever the hash says.  Nothing here calls the code
under test."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import numpy as np
import pyref as P
import verify_forge as F

HERE = os.path.dirname(os.path.abspath(__file__))
p, r = P.Q_MOD, P.R_MOD
DST_COMMITMENT, DST_FOLD = b"bsb22-commitment", b"G16-BSB22"
SHA_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128)
DST_LENGTHS = (1, 9, 16, 255)


def build_emu(so):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_decode.cpp")])
    return so


def bp(b):
    return C.cast(C.c_char_p(bytes(b)), C.c_void_p) if b is not None else None


# ---------------------------------------------------------------------------------------------------- hashes (RFC 9380 5.3.1, hashlib)
def expand_xmd48(msg, dst):
    H = lambda b: hashlib.sha256(b).digest()
    dstp = dst + bytes([len(dst)])
    b0 = H(bytes(64) + msg + (48).to_bytes(2, "big") + b"\0" + dstp)
    b1 = H(b0 + b"\1" + dstp)
    b2 = H(bytes(x ^ y for x, y in zip(b0, b1)) + b"\2" + dstp)
    return (b1 + b2)[:48]


def hash_to_field(msg, dst):
    return int.from_bytes(expand_xmd48(msg, dst), "big") % r


def bsb22_hashes(commitment_points, public_inputs, committed=None):
    """(values, fold): value_i = H(uncompressed C_i | full[j - 1] for j in committed[i]), full = public_inputs | values so far"""
    full, values = list(public_inputs), []
    committed = committed or [[] for _ in commitment_points]
    for c, js in zip(commitment_points, committed):
        v = hash_to_field(P.g1_uncompressed(c) + b"".join(full[j - 1].to_bytes(32, "big") for j in js), DST_COMMITMENT)
        values.append(v); full.append(v)
    fold = hash_to_field(b"".join(v.to_bytes(32, "big") for v in values), DST_FOLD) if values else None
    return values, fold


# ---------------------------------------------------------------------------------------------------- square roots by pow
def fp_is_residue(a):
    return a % p == 0 or pow(a, (p - 1) // 2, p) == 1


def fp2_has_root(a):
    """the norm test: a in Fp2 is a square iff a0^2 + a1^2 is one in Fp"""
    return fp_is_residue((a[0] * a[0] + a[1] * a[1]) % p)


def g1_y(x):
    """the two roots of x^3 + 3, or None"""
    t = (x * x * x + 3) % p
    y = pow(t, (p + 1) // 4, p)
    return y if y * y % p == t else None


def g1_decode_ref(b):
    """(point or None for infinity, malformed) of a 32-byte encoding, by the rules of include/mi355x_groth16_verify_bytes.h"""
    flag, x = b[0] >> 6, int.from_bytes(bytes([b[0] & 0x3F]) + b[1:], "big")
    if flag == 0:
        return None, True
    if flag == 1:
        return None, x != 0
    if x >= p or g1_y(x) is None:
        return None, True
    y = g1_y(x)
    if (y > (p - 1) // 2) != (flag == 3):
        y = p - y
    return (x, y), False


def twist_point_real_y(tries=64, seed=9):
    """a point of the twist with y.A1 = 0, or None: x^3 = t^2 - b' for seeded t in Fp.  p^2 - 1 = 3^k n with 3 not dividing n; the
    candidate x = c^(1/3 mod n) is a cube root of c exactly when c lies in the subgroup of order n (one c in 3^k), so it is kept only
    when x^3 really is c."""
    rnd = random.Random(seed)
    n = p * p - 1
    k = 0
    while n % 3 == 0:
        n //= 3; k += 1
    e = pow(3, -1, n)
    def f2pow(a, ex):
        acc = (1, 0)
        for bit in bin(ex)[2:]:
            acc = P.fp2_sqr(acc)
            if bit == "1":
                acc = P.fp2_mul(acc, a)
        return acc
    for _ in range(tries):
        t = rnd.randrange(1, p)
        c = P.fp2_sub((t * t % p, 0), P.G2_B)
        x = f2pow(c, e)
        if P.fp2_mul(P.fp2_sqr(x), x) == c:
            Q = (x, (t, 0))
            assert P.g2_is_on_curve(Q)
            return Q
    return None


def g1_edge_encodings():
    """[(name, 32 bytes, malformed)]: the refusals of the issue, each changing one thing, and the encodings that must be taken"""
    gen = P.g1_compress(P.G1_GEN)
    assert gen.hex() == "80" + "00" * 30 + "01"
    inf = P.g1_compress(None)
    x_no_y = next(x for x in range(2, 100) if g1_y(x) is None)
    out = [("generator", gen, False), ("-generator", P.g1_compress(P.g1_neg(P.G1_GEN)), False), ("infinity", inf, False),
           ("X = p", bytes([0x80 | (p >> 248)]) + (p % (1 << 248)).to_bytes(31, "big"), True),
           ("X = 2^254 - 1", bytes([0xBF]) + b"\xff" * 31, True), ("X = 0", bytes([0x80]) + bytes(31), True),
           ("X = 0, largest", bytes([0xC0]) + bytes(31), True),
           ("flag 00", bytes([gen[0] & 0x3F]) + gen[1:], True),
           ("flag 01, stray bit in the first byte", bytes([0x41]) + bytes(31), True),
           ("flag 01, stray bit in the last byte", bytes([0x40]) + bytes(30) + b"\1", True),
           ("X without y", bytes([0x80]) + x_no_y.to_bytes(32, "big")[1:], True)]
    assert p >> 254 == 0
    return out


def g2_edge_encodings():
    Q = P.g2_mul(P.G2_GEN, 5)
    enc = P.g2_compress(Q)
    pb = p.to_bytes(32, "big")
    out = [("generator", P.g2_compress(P.G2_GEN), False), ("-generator", P.g2_compress(P.g2_neg(P.G2_GEN)), False), ("infinity", P.g2_compress(None), False),
           ("only A1 >= p", bytes([0x80 | pb[0]]) + pb[1:] + enc[32:], True), ("only A0 >= p", enc[:32] + pb, True),
           ("A0 = 2^256 - 1", enc[:32] + b"\xff" * 32, True),
           ("flag 00", bytes([enc[0] & 0x3F]) + enc[1:], True),
           ("flag 01, stray bit in the first byte", bytes([0x41]) + bytes(63), True),
           ("flag 01, stray bit in the last byte", bytes([0x40]) + bytes(62) + b"\1", True),
           ("flag 01, stray bit in A0", bytes([0x40]) + bytes(31) + b"\x80" + bytes(31), True)]
    return out


def seeded_g1_encodings(n, seed):
    """n encodings with seeded X below 3 * 2^252 < p and a seeded sign flag: about half have no y"""
    rnd = random.Random(seed)
    return [bytes([rnd.choice((0x80, 0xC0)) | rnd.randrange(48)]) + rnd.randbytes(31) for _ in range(n)]


def seeded_g2_encodings(n, seed):
    rnd = random.Random(seed)
    return [bytes([rnd.choice((0x80, 0xC0)) | rnd.randrange(48)]) + rnd.randbytes(31) + bytes([rnd.randrange(48)]) + rnd.randbytes(31) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------- forged proofs that carry their hashes
def proof_bytes_of(case):
    pts = F.case_points(case)
    return P.proof_bytes({"ar": pts["ar"], "bs": pts["bs"], "krs": pts["krs"]}, pts["cm"], pts["pok"])


def rehashed(case, committed=None):
    """the case as the bytes path sees it: commitment values and fold challenge are the hashes of its commitments, whatever the case
    said; its other exponents stay.  A word of commitment_values / fold_challenge has no counterpart (those are no inputs here)."""
    pts = F.case_points(case)
    cv, fold = bsb22_hashes(pts["cm"], case["pub"], committed)
    return F.but(case, cv=cv, fold=fold, words=[w for w in case["words"] if w[0] not in ("commitment_values", "fold_challenge")])


def hashed_honest(key, seed, committed=None, **force):
    """an ACCEPTED proof whose values and challenge are the hashes: forge_proof solves krs and pok for them"""
    h = F.honest(key, seed, **force)
    cv, fold = bsb22_hashes([F.g1(m) for m in h["cm"]], h["pub"], committed)
    args = dict(force, commit_values=cv)
    if key["n_commitments"]:
        args["fold"] = fold
    c = F.honest(key, seed, **args)
    assert c["cm"] == h["cm"] and c["pub"] == h["pub"]
    return c


def has_no_encoding(case):
    """a non-reduced coordinate or a point off its curve cannot be written as compressed bytes"""
    return any(w[0] in ("raw", "pok", "commitments") for w in case["words"]) or case["malformed"] in ("off the curve", "off the twist")


def hashed_distinct_batch(key, n, seed, committed=None):
    """n accepted proofs of one key, each with its own inputs, as (bytes, public inputs, verdict) -- then some with one byte broken"""
    out = []
    for i in range(n):
        c = hashed_honest(key, seed + i, committed)
        out.append([proof_bytes_of(c), c["pub"], F.verdict_in_exponent(key, c)])
    return out
