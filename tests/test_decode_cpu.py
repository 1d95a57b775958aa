"""CPU suite: what reads a proof's bytes (gnark-whir_amd/csrc/decode_ops.cuh, sha256_h2f.cuh) in the host build (tests/emu/emu_decode.cpp,
-DMI_CHECK_NOWRAP) and through the library's host-only entry points (mi_proof_read, mi_hash_to_field): square roots in Fp and Fp2 on
their degenerate inputs, the point decoders on round trips and refusals, SHA-256 / expand_message_xmd / hash-to-field against hashlib,
whole proofs with known discrete logs whose commitment values and fold challenge are those hashes, and a stand-alone sanitizer build.
The references are Python only: hashlib, pow, oracle/pyref.py's encoders, tests/verify_forge.py's exponent rule."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import numpy as np
import pytest
import cref
import pyref as P
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import bytes_cases as BC
from helpers import fp_arr, fp_vals, fr_arr, fr_vals, g1_arr, g2_arr, g1_pts, g2_pts
from gpu_common import load_binding, ROOT

p, r = P.Q_MOD, P.R_MOD


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(BC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_decode.so")))


def _decode(emu, encs, g2=False):
    w = 64 if g2 else 32
    n = len(encs)
    out = np.zeros((n, w // 4), np.uint64); bad = np.zeros(n, np.uint8)
    fn = emu.emu_decode_g2 if g2 else emu.emu_decode_g1
    assert fn(b"".join(encs), C.c_size_t(n), V.p_(out), V.p_(bad)) == 0
    return out, bad


# ---------------------------------------------------------------------------------------------------- square roots
def test_fp_square_root_against_pow(emu):
    rnd = random.Random(3)
    vals = [0, 1, 4, 3, p - 1] + [rnd.randrange(p) for _ in range(60)]
    vals += [v * v % p for v in vals[5:25]]
    assert not BC.fp_is_residue(3) and not BC.fp_is_residue(p - 1) and BC.fp_is_residue(4)
    A = fp_arr(vals); Y = np.zeros_like(A); ok = np.zeros(len(vals), np.uint8)
    emu.emu_fp_sqrt(V.p_(Y), V.p_(A), C.c_size_t(len(vals)), V.p_(ok))
    ys = fp_vals(Y)
    assert 20 < int(ok.sum()) < len(vals) - 20
    for a, y, k in zip(vals, ys, ok):
        assert bool(k) == BC.fp_is_residue(a), a          # Euler's criterion
        assert y == pow(a, (p + 1) // 4, p)
        if k:
            assert y * y % p == a                            # the definitional check


def test_fp2_square_root_is_total(emu):
    """the four degenerate families (0; a1 = 0 with a0 a residue; a1 = 0 with a0 a non-residue, where the root is purely imaginary and
    the complex method divides by 0; a norm that is a non-residue) and seeded values: accept iff the norm is a residue, an accepted root
    squares back exactly"""
    rnd = random.Random(4)
    res = [v * v % p for v in (rnd.randrange(1, p) for _ in range(6))]
    non = [v for v in (rnd.randrange(1, p) for _ in range(40)) if not BC.fp_is_residue(v)][:6] + [3, p - 1]
    vals = [(0, 0)] + [(a, 0) for a in res + [1, 4]] + [(a, 0) for a in non] + [(0, a) for a in res[:3] + non[:3]]
    seeded = [(rnd.randrange(p), rnd.randrange(p)) for _ in range(40)]
    vals += seeded + [P.fp2_sqr(v) for v in seeded[:10]]
    no_root = [v for v in vals if not BC.fp2_has_root(v)]
    assert len(no_root) >= 10 and all(BC.fp2_has_root((a, 0)) for a in non)   # every element of Fp is a square in Fp2
    A = fp_arr([c for v in vals for c in v]).reshape(-1, 8); Y = np.zeros_like(A); ok = np.zeros(len(vals), np.uint8)
    emu.emu_fp2_sqrt(V.p_(Y), V.p_(A), C.c_size_t(len(vals)), V.p_(ok))
    ys = [tuple(fp_vals(row.reshape(2, 4))) for row in Y]
    for a, y, k in zip(vals, ys, ok):
        assert bool(k) == BC.fp2_has_root(a), a
        if k:
            assert P.fp2_sqr(y) == (a[0] % p, a[1] % p), a
            ref = V.fp2_sqrt(a)                               # the cross-check: the same root up to sign
            assert ref is not None and y in (ref, P.fp2_neg(ref))
    for a, y in zip(vals, ys):
        if a[1] == 0 and a[0] in non:
            assert y[0] == 0 and y[1] != 0                    # purely imaginary


# ---------------------------------------------------------------------------------------------------- decoding
def test_decode_inverts_compress(emu):
    rnd = random.Random(5)
    g1s = [P.g1_mul(P.G1_GEN, rnd.randrange(1, r)) for _ in range(12)]
    g1s += [P.g1_neg(q) for q in g1s] + [None, P.G1_GEN]
    out, bad = _decode(emu, [P.g1_compress(q) for q in g1s])
    assert not bad.any() and np.array_equal(out, g1_arr(g1s))
    assert {P.g1_compress(q)[0] >> 6 for q in g1s} == {1, 2, 3}
    g2s = [P.g2_mul(P.G2_GEN, rnd.randrange(1, 1 << 40)) for _ in range(6)]
    real_y = BC.twist_point_real_y(64)
    assert real_y is not None, "no twist point with y.A1 = 0 among 64 seeded t"
    g2s += [P.g2_neg(q) for q in g2s] + [None, P.G2_GEN, real_y, P.g2_neg(real_y), V.twist_point_outside_subgroup()]
    out, bad = _decode(emu, [P.g2_compress(q) for q in g2s], g2=True)
    assert not bad.any() and np.array_equal(out, g2_arr(g2s))
    assert P.g2_compress(real_y)[0] >> 6 != P.g2_compress(P.g2_neg(real_y))[0] >> 6


def test_decode_refusals_change_one_thing_each(emu):
    for g2, edges in ((False, BC.g1_edge_encodings()), (True, BC.g2_edge_encodings())):
        out, bad = _decode(emu, [e for _, e, _ in edges], g2=g2)
        for (name, _, want), b, row in zip(edges, bad, out):
            assert bool(b) == want, name
            if want:
                assert not row.any(), name
    assert sum(w for _, _, w in BC.g1_edge_encodings()) >= 8 and sum(w for _, _, w in BC.g2_edge_encodings()) >= 6


def test_decode_of_seeded_x_matches_python_both_ways(emu):
    encs = BC.seeded_g1_encodings(64, 6)
    out, bad = _decode(emu, encs)
    refs = [BC.g1_decode_ref(e) for e in encs]
    assert 16 <= sum(m for _, m in refs) <= 48
    for e, (pt, m), b, row in zip(encs, refs, bad, out):
        assert bool(b) == m and g1_pts(row) == [pt], e.hex()
        if not m:
            assert P.g1_compress(pt) == e
    encs2 = BC.seeded_g2_encodings(64, 7)
    out2, bad2 = _decode(emu, encs2, g2=True)
    assert 16 <= int(bad2.sum()) <= 48
    for e, b, row in zip(encs2, bad2, out2):
        x = (int.from_bytes(e[32:], "big"), int.from_bytes(bytes([e[0] & 0x3F]) + e[1:32], "big"))
        has = x[0] < p and x[1] < p and BC.fp2_has_root(P.fp2_add(P.fp2_mul(P.fp2_sqr(x), x), P.G2_B))
        assert bool(b) == (not has), e.hex()
        if has:
            (Q,) = g2_pts(row)
            assert P.g2_is_on_curve(Q) and Q[0] == x and P.g2_compress(Q) == e


# ---------------------------------------------------------------------------------------------------- SHA-256 and hash-to-field
def test_sha256_against_hashlib_at_the_padding_edges(emu):
    out = C.create_string_buffer(32)
    for msg, lit in ((b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
                     (b"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")):
        emu.emu_sha256(msg, C.c_size_t(len(msg)), out)
        assert out.raw.hex() == lit
    rnd = random.Random(8)
    for n in BC.SHA_LENGTHS + (13, 20, 45, 52, 1000):
        msg = rnd.randbytes(n)
        emu.emu_sha256(msg, C.c_size_t(n), out)
        assert out.raw == hashlib.sha256(msg).digest(), n


def test_hash_to_field_against_python(emu):
    B = load_binding()
    rnd = random.Random(9)
    x48 = C.create_string_buffer(48)
    for dl in BC.DST_LENGTHS:
        dst = rnd.randbytes(dl)
        for n in BC.SHA_LENGTHS:
            msg = rnd.randbytes(n)
            emu.emu_expand_xmd48(dst, C.c_uint(dl), msg, C.c_size_t(n), x48)
            assert x48.raw == BC.expand_xmd48(msg, dst), (dl, n)
            got = np.zeros((1, 4), np.uint64)
            emu.emu_hash_to_field(dst, C.c_uint(dl), msg, C.c_size_t(n), C.c_size_t(1), V.p_(got))
            assert fr_vals(got) == [BC.hash_to_field(msg, dst)], (dl, n)
            assert np.array_equal(B.hash_to_field(dst, msg), got[0])
    # the reduction alone: all ff, values congruent to 0 mod r, the edges of the conditional subtractions
    for v in [(1 << 384) - 1, 0, r, 5 * r, r << 128, (1 << 256) - 1, 1 << 256, (1 << 256) + r - 1, r - 1, 5 * r - 1, 5 * r + 1, ((1 << 384) // r) * r]:
        got = np.zeros((1, 4), np.uint64)
        emu.emu_fr_from_be48(v.to_bytes(48, "big"), V.p_(got))
        assert fr_vals(got) == [v % r] and cref.limbs_to_int(got[0]) < r, hex(v)
    assert B.load().mi_hash_to_field(b"x", C.c_size_t(0), b"", C.c_size_t(0), V.p_(np.zeros(4, np.uint64))) == -1
    assert B.load().mi_hash_to_field(bytes(256), C.c_size_t(256), b"", C.c_size_t(0), V.p_(np.zeros(4, np.uint64))) == -1
    assert B.load().mi_hash_to_field(b"x", C.c_size_t(1), b"", C.c_size_t(0), None) == -1


# ---------------------------------------------------------------------------------------------------- whole proofs
@pytest.mark.parametrize("nc", [0, 1, 2])
def test_proof_read_inverts_proof_write(nc):
    B = load_binding()
    g1 = cref.gen_g1(8, 30 + nc); g2 = cref.gen_g2(2, 31)
    raw = np.concatenate([g1[0], g2[0], g1[1]])
    cm, pok = g1[2:2 + nc].copy(), g1[6].copy()
    data = B.proof_write(raw, commitments=cm if nc else None, pok=pok)
    assert len(data) == 164 + 32 * nc
    got = B.proof_read(data, nc)
    assert got is not None and np.array_equal(got[0], raw) and np.array_equal(got[1], cm) and np.array_equal(got[2], pok)
    assert B.proof_read(data, nc + 1) is None and B.proof_read(data[:-1], nc) is None and B.proof_read(data + b"\0", nc) is None
    wrong_count = data[:128] + (nc + 1).to_bytes(4, "big") + data[132:]
    assert B.proof_read(wrong_count, nc) is None
    inf = B.proof_write(np.zeros(32, np.uint64), commitments=np.zeros((nc, 8), np.uint64) if nc else None, pok=None)
    got = B.proof_read(inf, nc)
    assert got is not None and not got[0].any() and not got[1].any() and not got[2].any()
    lib = B.load()
    assert lib.mi_proof_read(None, C.c_size_t(164), C.c_uint32(0), V.p_(raw), None, V.p_(pok)) == -1
    assert lib.mi_proof_read(data, C.c_size_t(len(data)), C.c_uint32(nc), None, None, None) == -1


def test_every_flipped_byte_changes_the_points_or_is_refused():
    B = load_binding()
    g1 = cref.gen_g1(4, 40); g2 = cref.gen_g2(1, 41)
    raw = np.concatenate([g1[0], g2[0], g1[1]])
    data = B.proof_write(raw, commitments=g1[2:3].copy(), pok=g1[3].copy())
    assert len(data) == 196
    base = B.proof_read(data, 1)
    refused = 0
    for i in range(196):
        for mask in (0x01, 0x80, 0xFF):
            mut = bytearray(data); mut[i] ^= mask
            got = B.proof_read(bytes(mut), 1)
            if got is None:
                refused += 1
            else:
                assert not all(np.array_equal(a, b) for a, b in zip(got, base)), (i, mask)
    assert 100 < refused < 3 * 196 - 100


@pytest.fixture(scope="module")
def judge(emu):
    """(key, proof bytes, public inputs, committed lists) -> (verdict of emu_verify_bytes, the decoded words)"""
    keys = {}

    def run(key, data, pub, committed=None, proof_len=None):
        if key["id"] not in keys:
            d, nbp, ped = V.vk_arrays(key["vk"])
            eab = np.zeros((1, 48), np.uint64)
            assert emu.emu_pairing_one(V.p_(d["alpha1"]), V.p_(d["beta2"]), V.p_(eab)) == 0
            keys[key["id"]] = (d, nbp, ped, eab)
        d, nbp, ped, eab = keys[key["id"]]
        nc = key["n_commitments"]
        lists = committed or [[] for _ in range(nc)]
        off = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32); idx = np.array([j for l in lists for j in l] + [0], np.uint32)
        dec = np.zeros((4 + nc) * 8 + 8, np.uint64)
        pubs = fr_arr(pub) if pub else None
        v = emu.emu_verify_bytes(V.p_(d["k"]), V.p_(d["gamma2"]), V.p_(d["delta2"]), V.p_(ped), C.c_uint(nbp), C.c_uint(nc), V.p_(eab), data,
                                 C.c_size_t(len(data) if proof_len is None else proof_len), V.p_(pubs), V.p_(off), V.p_(idx), V.p_(dec))
        return v, dec
    return run


def _flip_sign(data, off):
    assert data[off] >> 6 in (2, 3)
    return data[:off] + bytes([data[off] ^ 0x40]) + data[off + 1:]


@pytest.mark.parametrize("shape", [(2, 0), (3, 1), (3, 3)])
def test_forged_proofs_with_hashed_values_through_the_host_half(judge, shape):
    key = F.forge_key(*shape)
    nc = shape[1]
    c = BC.hashed_honest(key, 200 + nc)
    assert F.verdict_in_exponent(key, c) == R.OK
    data = BC.proof_bytes_of(c)
    v, dec = judge(key, data, c["pub"])
    assert v == R.OK
    inp = F.verify_input(c)
    want = np.concatenate([inp["raw"]] + ([inp["commitments"].reshape(-1), inp["pok"]] if nc else [np.zeros(8, np.uint64)]))
    assert np.array_equal(dec, want)
    assert judge(key, _flip_sign(data, 0), c["pub"])[0] == R.PAIRING            # -Ar: a well-formed proof of something else
    assert judge(key, data, [(c["pub"][0] + 1) % r] + c["pub"][1:])[0] == R.PAIRING
    bad_count = data[:128] + (nc + 1).to_bytes(4, "big") + data[132:]
    assert judge(key, bad_count, c["pub"])[0] == R.MALFORMED
    assert judge(key, data, c["pub"], proof_len=len(data) - 1)[0] == -1
    if nc:
        assert judge(key, _flip_sign(data, 132), c["pub"])[0] == R.PAIRING       # -C_0: its hash changes, and kSum with it
        flipped = F.but(c, cm=[-c["cm"][0] % r] + c["cm"][1:])
        assert F.verdict_in_exponent(key, BC.rehashed(flipped)) == R.PAIRING
        assert judge(key, data[:132] + bytes([0x80]) + bytes(31) + data[164:], c["pub"])[0] == R.MALFORMED   # X = 0: no point


def test_public_committed_lists_reach_the_hash(judge, emu):
    """commitment 1 commits public wire 1 and commitment 0's value: other values than with empty lists, and the verdict follows"""
    key = F.forge_key(3, 3)
    lists = [[], [1, 3], [2]]
    c0, c1 = BC.hashed_honest(key, 300), BC.hashed_honest(key, 300, committed=lists)
    assert c0["cm"] == c1["cm"] and c0["cv"][0] == c1["cv"][0] and c0["cv"][1] != c1["cv"][1] and c0["cv"][2] != c1["cv"][2]
    for c, l, other in ((c0, None, lists), (c1, lists, None)):
        data = BC.proof_bytes_of(c)
        assert judge(key, data, c["pub"], l)[0] == R.OK == F.verdict_in_exponent(key, c)
        assert judge(key, data, c["pub"], other)[0] == R.PAIRING == F.verdict_in_exponent(key, BC.rehashed(c, other))
    # the hash body alone against Python
    pts = F.case_points(c1)
    off = np.array([0, 0, 2, 3], np.uint32); idx = np.array([1, 3, 2], np.uint32)
    vals = np.zeros((3, 4), np.uint64); fold = np.zeros(4, np.uint64)
    emu.emu_bsb22_hashes(V.p_(g1_arr(pts["cm"])), C.c_uint(3), V.p_(fr_arr(c1["pub"])), C.c_uint(2), V.p_(off), V.p_(idx), V.p_(vals), V.p_(fold))
    assert fr_vals(vals) == c1["cv"] and fr_vals(fold) == [c1["fold"]]
    inf_first = BC.bsb22_hashes([None] + pts["cm"][1:], c1["pub"], lists)
    emu.emu_bsb22_hashes(V.p_(g1_arr([None] + pts["cm"][1:])), C.c_uint(3), V.p_(fr_arr(c1["pub"])), C.c_uint(2), V.p_(off), V.p_(idx), V.p_(vals), V.p_(fold))
    assert fr_vals(vals) == inf_first[0] and fr_vals(fold) == [inf_first[1]]   # infinity hashes as 64 zero bytes


# ---------------------------------------------------------------------------------------------------- the sanitizer build
def test_mutated_and_truncated_bytes_never_trip_a_sanitizer():
    """tests/cpp/decode_fuzz.cpp, its own main, -fsanitize=address,undefined on the host: mi_proof_read and the decoders over seeded
    mutated and truncated strings of every length from 0 to 164 + 32 * 17"""
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-decode"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "decode_fuzz_asan"), "7"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    accepted, refused = (int(x) for x in res.stdout.split()[-2:])
    assert accepted > 50 and refused > 1000


def test_the_staged_batch_of_the_verifier_never_trips_a_sanitizer():
    """tests/cpp/verify_stage_asan.cpp, its own main, -fsanitize=address,undefined -DMI_CHECK_NOWRAP on the host: VerifyStage
    (csrc/pairing_ops.cuh) over exactly-sized heap arrays -- four keys, batches of 0, 1 and 3, four variants each: null optional
    pointers, proofs flagged by decode_malformed with every pointer null, words that are not reduced -- with the flags, the first
    flagged index and every scalar row checked inside the program"""
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-stage"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "verify_stage_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    assert int(res.stdout.split()[-1]) == 4 * 3 * 4
