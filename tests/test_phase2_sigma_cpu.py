"""CPU suite: the sigma chain of a phase-2 ceremony on the host (include/mi355x_groth16_phase2_check.h): the steps that re-randomise the
points [-sigma_k]2 of a state, each a Schnorr proof per commitment over the twist under one challenge.  The chain is restated in
tests/phase2_sigma_ref.py (hashlib, oracle/pyref.py's group law); the restated steps go through the shared library's
mi_phase2_sigma_records_verify, and tests/cpp/phase2_sigma_host.cpp -- its own main, built with -fsanitize=address,undefined by
`make sanitize-phase2-sigma` -- makes the same steps with csrc/ceremony_ops.cuh and verifies them over heap blocks of exactly their
size.  No library is preloaded anywhere."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest
import pyref as P
import phase2_sigma_ref as S
from helpers import fr_arr, g2_arr
from gpu_common import load_binding, ROOT

R = P.R_MOD
HEADER = os.path.join(ROOT, "include", "mi355x_groth16_phase2_check.h")
ID0 = bytes(32)
ID1 = hashlib.sha256(b"a transcript").digest()
FULL = 0x2A3C09F0A58A7E85_00E0A7EB8EF62ABC_402D111E41112ED4_9BD61B6E725B19F1 % R
E_START = [R - 11, R - FULL]   # g_sigma_neg_k = [-sigma_k]2 for sigma = 11 and a full-width value
# (s, nonce) per commitment of three steps: full-width values, a small factor, a nonce of r - 1, a factor of r - 2
STEPS = [[(FULL, 0x1F3A9C5D7E2B4681_0FEDCBA987654321_1122334455667788 % R), (3, R - 1)],
         [(R - 2, FULL * 7 % R), (FULL * 5 % R, 12345)],
         [(7, FULL * 11 % R), (FULL * 3 % R, FULL * 13 % R)]]
SHAPES = [(nc, m, ident, first) for nc in (1, 2) for m in (1, 3) for ident, first in ((ID0, 0), (ID1, 5))]


@pytest.fixture(scope="module")
def chains():
    """every (nc, m, id, first_index) chain restated once: (steps, the exponents after the last step)"""
    return {(nc, m, ident, first): S.chain(ident, first, E_START[:nc], [st[:nc] for st in STEPS[:m]]) for nc, m, ident, first in SHAPES}


def start_of(nc):
    return g2_arr([P.g2_mul(P.G2_GEN, e) for e in E_START[:nc]])


def test_restatement_accepts_its_own_steps_and_no_tampered_one(chains):
    """the yardstick itself: the acceptance rule, stated apart from the making of a step, holds for every step and fails for a response + 1"""
    steps, e_end = chains[(2, 3, ID1, 5)]
    befores, prev = [P.g2_mul(P.G2_GEN, e) for e in E_START], ID1
    for i, (parts, h) in enumerate(steps):
        assert S.accepts(prev, 5 + i, befores, parts, h)
        assert not S.accepts(prev, 5 + i, befores, [(parts[0][0], parts[0][1], (parts[0][2] + 1) % R), parts[1]], h)
        assert not S.accepts(prev, 6 + i, befores, parts, h)
        befores, prev = [p[0] for p in parts], h
    want = [e * s0 % R * s1 % R * s2 % R for e, (s0, s1, s2) in zip(E_START, zip(*[[s for s, _ in st] for st in STEPS]))]
    assert e_end == want and befores == [P.g2_mul(P.G2_GEN, e) for e in e_end]


@pytest.mark.parametrize("nc,m,ident,first", SHAPES, ids=[f"nc{nc}-m{m}-first{first}" for nc, m, _, first in SHAPES])
def test_restated_sigma_chain_verifies_through_the_library(chains, nc, m, ident, first):
    B = load_binding()
    steps, _ = chains[(nc, m, ident, first)]
    pr, hs = S.proofs_array(steps)
    start = start_of(nc)
    verify = lambda p=pr, h=hs, st=start, idn=ident, f=first: B.phase2_sigma_records_verify(st, idn, f, p, h)
    assert verify() == m
    assert verify(p=pr[:0], h=[]) == 0
    if m > 1:   # a chain verified in two pieces: the second continues where the first ended
        assert verify(p=pr[:1], h=hs[:1]) == 1
        assert verify(p=pr[1:], h=hs[1:], st=pr[0, :, :16], idn=hs[0], f=first + 1) == m - 1
    other = g2_arr([P.g2_mul(P.G2_GEN, 5)])[0]
    r_words = np.frombuffer(R.to_bytes(32, "little"), np.uint64)
    for i in range(m):
        t = list(hs); t[i] = bytes([t[i][0] ^ 0x40]) + t[i][1:]
        assert verify(h=t) == i, "one byte of a hash"
        for k in range(nc):   # the same index whichever commitment of the step is hit
            t = pr.copy(); t[i, k, :16] = other
            assert verify(p=t) == i, "after replaced"
            t = pr.copy(); t[i, k, 16:32] = other
            assert verify(p=t) == i, "commit replaced"
            t = pr.copy(); t[i, k, 32:] = fr_arr([(steps[i][0][k][2] + 1) % R])[0]
            assert verify(p=t) == i, "response + 1"
            t = pr.copy(); z = int.from_bytes(t[i, k, 32:].tobytes(), "little") + R
            assert z < 1 << 256
            t[i, k, 32:] = np.frombuffer(z.to_bytes(32, "little"), np.uint64)
            assert verify(p=t) == i, "response + r: the same element in words that are not below r"
            t = pr.copy(); t[i, k, 32:] = r_words
            assert verify(p=t) == i, "a response of r"
            for lo in (0, 16):
                t = pr.copy(); t[i, k, lo] ^= np.uint64(1)
                assert verify(p=t) == i, "a point moved off the twist"
                t = pr.copy(); t[i, k, lo:lo + 16] = 0
                assert verify(p=t) == i, "a point at infinity"
    if m > 1:
        assert verify(p=pr[[1, 0, 2]], h=[hs[1], hs[0], hs[2]]) == 0, "steps swapped"
        assert verify(p=pr[[0, 2, 1]], h=[hs[0], hs[2], hs[1]]) == 1, "steps swapped"
    if nc > 1:
        assert verify(p=pr[:, ::-1]) == 0, "the commitments of every step swapped"
    assert verify(f=first + 1) == 0, "wrong first_index"
    assert verify(idn=bytes([ident[0] ^ 1]) + ident[1:]) == 0, "wrong start_hash"
    wrong = start.copy(); wrong[nc - 1] = other
    assert verify(st=wrong) == 0, "wrong start point"


def test_sigma_records_verify_refusals(chains):
    B = load_binding()
    lib = B.load()
    steps, _ = chains[(2, 3, ID0, 0)]
    pr, hs = S.proofs_array(steps)
    start = start_of(2)
    for k in range(2):
        off = start.copy(); off[k, 4] ^= np.uint64(1)
        inf = start.copy(); inf[k] = 0
        for bad in (off, inf):
            with pytest.raises(B.MiError):
                B.phase2_sigma_records_verify(bad, ID0, 0, pr, hs)
    # null pointers and nc = 0, through the C-ABI directly; first_bad is not written
    hbuf = (C.c_uint8 * 96).from_buffer_copy(b"".join(hs))
    sp, pp = start.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p)
    call = lambda st, nc, sh, p, h, m, fb: lib.mi_phase2_sigma_records_verify(st, C.c_uint32(nc), sh, C.c_uint64(0), p, h, C.c_size_t(m), fb)
    fb = C.c_uint64(77)
    assert call(sp, 2, ID0, pp, hbuf, 3, C.byref(fb)) == 0 and fb.value == 3
    fb = C.c_uint64(77)
    for args in ((None, 2, ID0, pp, hbuf, 3, C.byref(fb)), (sp, 0, ID0, pp, hbuf, 3, C.byref(fb)), (sp, 2, None, pp, hbuf, 3, C.byref(fb)),
                 (sp, 2, ID0, None, hbuf, 3, C.byref(fb)), (sp, 2, ID0, pp, None, 3, C.byref(fb)), (sp, 2, ID0, pp, hbuf, 3, None)):
        assert call(*args) == -1 and fb.value == 77
    assert call(sp, 2, ID0, None, None, 0, C.byref(fb)) == 0 and fb.value == 0   # proofs and hashes may be null with m = 0


def run_host(lines):
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-phase2-sigma"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "phase2_sigma_host_asan")], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                         env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    return res.stdout.splitlines()


def point_line(pt):
    return "inf" if pt is None else f"{pt[0][0]:064x} {pt[0][1]:064x} {pt[1][0]:064x} {pt[1][1]:064x}"


# (tamper, step, commitment, rc, first_bad) over the chain of two commitments and three steps
HOST_TAMPERS = [("none", 0, 0, 0, 3), ("response", 0, 0, 0, 0), ("response", 2, 1, 0, 2), ("responser", 1, 0, 0, 1), ("responser", 1, 1, 0, 1), ("commit", 1, 1, 0, 1),
                ("after", 0, 1, 0, 0), ("after", 2, 0, 0, 2), ("offtwist", 1, 0, 0, 1), ("offtwist", 2, 1, 0, 2), ("infinity", 0, 1, 0, 0), ("infinity", 2, 0, 0, 2),
                ("hashbyte", 1, 0, 0, 1), ("swap", 0, 0, 0, 0), ("swap", 1, 0, 0, 1), ("index", 0, 0, 0, 0), ("starthash", 0, 0, 0, 0),
                ("null", 0, 0, -1, (1 << 64) - 1), ("nczero", 0, 0, -1, (1 << 64) - 1), ("startinf", 0, 1, -1, (1 << 64) - 1), ("startoff", 0, 0, -1, (1 << 64) - 1)]


def test_sigma_chain_on_the_host_under_the_sanitizers(chains):
    """the stand-alone driver makes the steps with csrc/ceremony_ops.cuh (byte for byte the restated ones) and verifies them, tampered or
    not, over heap blocks of exactly m * nc proofs and m hashes"""
    cases = [(2, 3, ident, first, t) for ident, first in ((ID0, 0), (ID1, 5)) for t in HOST_TAMPERS] + [(1, 1, ID1, 5, HOST_TAMPERS[0][:4] + (1,)), (1, 1, ID0, 0, ("response", 0, 0, 0, 0))]
    lines = []
    for nc, m, ident, first, (tamper, i, k, _, _) in cases:
        flat = " ".join(f"{s:x} {n:x}" for st in STEPS[:m] for s, n in st[:nc])
        lines.append(f"sigma {ident.hex()} {first:x} {nc} {' '.join(f'{e:x}' for e in E_START[:nc])} {m} {flat} {tamper} {i} {k}")
    lines.append(f"sigma {ID0.hex()} 0 2 {E_START[0]:x} {E_START[1]:x} 0 none 0 0")   # no step: all of none hold
    out = run_host(lines)
    at = 0
    for n, (nc, m, ident, first, (tamper, i, k, rc, first_bad)) in enumerate(cases):
        assert out[at] == lines[n]
        at += 1
        for parts, h in chains[(nc, m, ident, first)][0]:
            for after, commit, z in parts:
                assert out[at:at + 3] == [point_line(after), point_line(commit), f"{z:064x}"], (tamper, first)
                at += 3
            assert out[at] == h.hex()
            at += 1
        assert out[at] == f"rc {rc} first_bad {first_bad}", (nc, m, tamper, i, k, out[at])
        at += 1
    assert out[at + 1] == "rc 0 first_bad 0" and at + 2 == len(out)


def test_sigma_header_and_binding_agree():
    B = load_binding()
    lib = B.load()
    src = open(HEADER).read()
    assert B.PHASE2_SIGMA_PROOF_WORDS * 8 == 128 + 128 + 32 == S.WORDS * 8 and C.sizeof(B.Phase2SigmaClaim) == 3 * 8 and C.sizeof(B.Phase2ChainInfo) == 8 + 2 * (8 + 32)
    for name in ("SIGMA_RECORD", "SIGMA_LINK", "BES"):
        assert int(re.search(rf"#define MI_PHASE2_BAD_{name}\s+(\d+)u", src).group(1)) == getattr(B, "PHASE2_BAD_" + name)
    for n in ("mi_phase2_get_pedersen_vk", "mi_phase2_contribute_sigma_proved", "mi_phase2_sigma_records_verify", "mi_phase2_get_chain_info", "mi_phase2_verify_adopt_sigma"):
        assert n in B.PHASE2_CHECK_EXPORTS and hasattr(lib, n) and re.search(rf"\b{n}\s*\(", src), n
    flat = " ".join(src.split())
    for phrase in ("mi355x-phase2-sigma-record", "mi355x-phase2-sigma-challenge", "le32(n_commitments)", "compress2 = mi_g2_compress", "SIGMA HAS A CHAIN OF ITS OWN"):
        assert phrase in flat, phrase
    for gone in ("has no proof of knowledge and no chain", "who knows sigma it cannot say"):
        assert gone not in flat, gone
