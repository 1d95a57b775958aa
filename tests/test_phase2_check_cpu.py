"""CPU suite: the host side of the ceremony checks (include/mi355x_groth16_phase2_check.h).  tests/cpp/phase2_check_host.cpp, its own
main, built with -fsanitize=address,undefined by `make sanitize-phase2-check`, runs the coefficient of a same-ratio test, the hash and
the challenge of a contribution's record and the making of a record (csrc/ceremony_ops.cuh) and mi_phase2_records_verify
(csrc/phase2_records.hip).  What it prints is compared here with hashlib and with oracle/pyref.py's own group law: the records are
restated from the exponents in Python integers.  No library is preloaded anywhere.  The same chain then goes through the shared
library's mi_phase2_records_verify, and the library's exports and the binding's structures are compared with the header."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest
import pyref as P
from helpers import fr_arr, g1_arr
from gpu_common import load_binding, ROOT

R = P.R_MOD
HEADER = os.path.join(ROOT, "include", "mi355x_groth16_phase2_check.h")
SEED = bytes(range(7, 39))
ID0 = bytes(32)
ID1 = hashlib.sha256(b"a transcript").digest()
FULL = 0x2A3C09F0A58A7E85_00E0A7EB8EF62ABC_402D111E41112ED4_9BD61B6E725B19F1 % R
# (d, nonce) of three contributions: full-width values, a small delta, a nonce of r - 1
STEPS = [(FULL, 0x1F3A9C5D7E2B4681_0FEDCBA987654321_1122334455667788 % R), (3, R - 1), (R - 2, FULL * 7 % R)]
START = 11   # delta1 before the first record = 11 g1


def coeff(seed, k):
    return int.from_bytes(hashlib.sha256(b"mi355x-ceremony-coeff" + seed + k.to_bytes(8, "little")).digest()[:16], "little")


def record_hash(prev, index, before, after, commit):
    return hashlib.sha256(b"mi355x-phase2-record" + prev + index.to_bytes(8, "little") + P.g1_compress(before) + P.g1_compress(after)
                          + P.g1_compress(commit)).digest()


def challenge(h):
    return int.from_bytes(hashlib.sha256(b"mi355x-phase2-challenge" + h).digest()[:16], "little")


def chain(ident, first_index, e_start, steps):
    """the records of `steps` restated: [(delta1, commit, response, hash)] with the points from pyref's group law"""
    out = []
    e, prev = e_start, ident
    for i, (d, k) in enumerate(steps):
        before, after, commit = P.g1_mul(P.G1_GEN, e), P.g1_mul(P.G1_GEN, e * d % R), P.g1_mul(P.G1_GEN, e * k % R)
        h = record_hash(prev, first_index + i, before, after, commit)
        out.append((after, commit, (k + challenge(h) * d) % R, h))
        e, prev = e * d % R, h
    return out


def records_array(recs):
    """the restated records as the library's words: (m, 24) uint64"""
    out = np.zeros((len(recs), 24), np.uint64)
    for i, (after, commit, z, h) in enumerate(recs):
        out[i, :8] = g1_arr([after])[0]
        out[i, 8:16] = g1_arr([commit])[0]
        out[i, 16:20] = fr_arr([z])[0]
        out[i, 20:] = np.frombuffer(h, np.uint64)
    return out


def run_host(lines):
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-phase2-check"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "phase2_check_host_asan")], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                         env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    return res.stdout.splitlines()


def point_line(pt):
    return "inf" if pt is None else f"{pt[0]:064x} {pt[1]:064x}"


# (tamper, index, first_bad): each single tamper is rejected at the record it touches; a wrong first_index or start_hash at record 0
TAMPERS = [("none", 0, 3), ("response", 0, 0), ("response", 2, 2), ("commit", 1, 1), ("delta1", 0, 0), ("delta1", 2, 2), ("hashbyte", 1, 1), ("hashbyte", 2, 2),
           ("swap", 0, 0), ("swap", 1, 1), ("index", 0, 0), ("starthash", 0, 0)]


def test_ceremony_hashes_records_and_chain_on_the_host():
    ks = [0, 1, (1 << 24) - 1, 1 << 40]
    lines = [f"coeff {SEED.hex()} {k:x}" for k in ks]
    hash_cases = [(ID0, 0, 5, 7, 9), (ID1, (1 << 40) + 3, FULL, R - 1, 1)]
    lines += [f"hash {i.hex()} {idx:x} {a:x} {b:x} {c:x}" for i, idx, a, b, c in hash_cases]
    steps = " ".join(f"{d:x} {k:x}" for d, k in STEPS)
    chains = [(ident, first, t) for ident, first in ((ID0, 0), (ID1, 5)) for t in TAMPERS]
    lines += [f"chain {ident.hex()} {first:x} {START:x} {len(STEPS)} {steps} {t[0]} {t[1]}" for ident, first, t in chains]
    lines.append(f"chain {ID0.hex()} 0 {START:x} 0 none 0")           # no record: all of none hold
    lines.append(f"chain {ID0.hex()} 0 {START:x} {len(STEPS)} {steps} null 0")
    out = run_host(lines)
    at = 0
    for n, k in enumerate(ks):
        assert out[at] == lines[n] and int(out[at + 1], 16) == coeff(SEED, k), f"r_{k}"
        at += 2
    for ident, idx, a, b, c in hash_cases:
        h = record_hash(ident, idx, *(P.g1_mul(P.G1_GEN, e) for e in (a, b, c)))
        assert out[at + 1] == h.hex() and int(out[at + 2], 16) == challenge(h)
        at += 3
    for n, (ident, first, (tamper, _, first_bad)) in enumerate(chains):
        want = chain(ident, first, START, STEPS)
        assert out[at] == lines[len(ks) + len(hash_cases) + n]
        for after, commit, z, h in want:
            assert out[at + 1:at + 5] == [point_line(after), point_line(commit), f"{z:064x}", h.hex()], (tamper, first)
            at += 4
        assert out[at + 1] == f"rc 0 first_bad {first_bad}", (tamper, first, out[at + 1])
        at += 2
    assert out[at + 1] == "rc 0 first_bad 0"
    at += 2
    assert out[at + 1 + 4 * len(STEPS)] == f"rc -1 first_bad {(1 << 64) - 1}"   # a null argument: MI_EINVAL, nothing written
    assert at + 2 + 4 * len(STEPS) == len(out)


def test_restated_records_verify_through_the_library():
    """the records restated in Python (pyref's points, hashlib's hashes) hold for the shared library's mi_phase2_records_verify, and
    each tamper made on this side is rejected where it is made"""
    B = load_binding()
    for ident, first in ((ID0, 0), (ID1, 5)):
        want = chain(ident, first, START, STEPS)
        recs = records_array(want)
        start = g1_arr([P.g1_mul(P.G1_GEN, START)])[0]
        assert B.phase2_records_verify(start, ident, first, recs) == 3
        assert B.phase2_records_verify(start, ident, first, recs[:0]) == 0
        # a chain verified in two pieces: the second continues where the first ended
        assert B.phase2_records_verify(start, ident, first, recs[:1]) == 1
        assert B.phase2_records_verify(recs[0, :8], recs[0, 20:].tobytes(), first + 1, recs[1:]) == 2
        for i in range(3):
            t = recs.copy(); t[i, 16:20] = fr_arr([(want[i][2] + 1) % R])[0]
            assert B.phase2_records_verify(start, ident, first, t) == i, "response + 1"
            t = recs.copy(); t[i, 8:16] = g1_arr([P.g1_mul(P.G1_GEN, 5)])[0]
            assert B.phase2_records_verify(start, ident, first, t) == i, "commit replaced"
            t = recs.copy(); t[i, :8] = g1_arr([P.g1_mul(P.G1_GEN, 5)])[0]
            assert B.phase2_records_verify(start, ident, first, t) == i, "delta1 replaced"
            t = recs.copy(); t[i, 21] ^= np.uint64(1 << 9)
            assert B.phase2_records_verify(start, ident, first, t) == i, "one byte of the hash"
            t = recs.copy(); t[i, 0] ^= np.uint64(1)
            assert B.phase2_records_verify(start, ident, first, t) == i, "delta1 off the curve"
            t = recs.copy(); t[i, 8:16] = 0
            assert B.phase2_records_verify(start, ident, first, t) == i, "commit at infinity"
            t = recs.copy(); t[i, 16:20] = np.frombuffer(R.to_bytes(32, "little"), np.uint64)
            assert B.phase2_records_verify(start, ident, first, t) == i, "a response that is not below r"
        assert B.phase2_records_verify(start, ident, first, recs[[1, 0, 2]]) == 0, "records swapped"
        assert B.phase2_records_verify(start, ident, first, recs[[0, 2, 1]]) == 1, "records swapped"
        assert B.phase2_records_verify(start, ident, first + 1, recs) == 0, "wrong first_index"
        assert B.phase2_records_verify(start, bytes([ident[0] ^ 1]) + ident[1:], first, recs) == 0, "wrong start_hash"
        assert B.phase2_records_verify(g1_arr([P.g1_mul(P.G1_GEN, START + 1)])[0], ident, first, recs) == 0, "wrong start point"
        off = start.copy(); off[4] ^= np.uint64(1)
        for bad_start in (np.zeros(8, np.uint64), off):   # infinity, off the curve
            with pytest.raises(B.MiError):
                B.phase2_records_verify(bad_start, ident, first, recs)


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_phase2_check_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert "mi_srs_check_powers" in names and "mi_phase2_verify_adopt" in names and "mi_phase2_records_verify" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_phase2_check.h but not exported"
    assert sorted(B.PHASE2_CHECK_EXPORTS) == names
    assert not set(B.PHASE2_CHECK_EXPORTS) & (set(B.EXPORTS) | set(B.PHASE2_EXPORTS))
    assert hasattr(lib, "mi_debug_ceremony_coeffs_dev")


def test_phase2_check_header_and_binding_agree():
    B = load_binding()
    src = open(HEADER).read()
    assert C.sizeof(B.SrsCheckStats) == 7 * 4 + 4 + 8 and C.sizeof(B.Phase2Claim) == 4 * 8 + 64 + 128 and B.PHASE2_RECORD_WORDS * 8 == 64 + 64 + 32 + 32
    for name in ("GENERATORS", "TAU_G1", "ALPHA_G1", "BETA_G1", "TAU_G2", "BETA_G2"):
        assert int(re.search(rf"#define MI_SRS_BAD_{name}\s+(\d+)u", src).group(1)) == getattr(B, "SRS_BAD_" + name)
    for name in ("RECORD", "DELTA", "Z", "K"):
        assert int(re.search(rf"#define MI_PHASE2_BAD_{name}\s+(\d+)u", src).group(1)) == getattr(B, "PHASE2_BAD_" + name)
    flat = " ".join(src.split())
    for phrase in ("A SEED THE MAKER OF THE DATA CANNOT PREDICT", "THIS PROJECT'S OWN FORMAT", "NOT COVERED", "BasisExpSigma", "phase-1 transcript",
                   "will not verify for anyone else"):
        assert phrase in flat, phrase
    assert "mi355x_groth16_debug.h" not in src and not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
