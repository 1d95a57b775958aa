"""CPU suite of the key-file entry points (include/mi355x_groth16_keyfile.h): the host-only inspector of both encodings on streams written
in Python (tests/keyfile_cases.py), its sanitizer build (gnark-whir_amd/Makefile `sanitize-keyfile`, its own main, nothing preloaded), and
the per-point text of the bulk kernels (gnark-whir_amd/csrc/keyfile_ops.cuh) in the host build tests/emu/emu_keyfile.cpp with
-DMI_CHECK_NOWRAP: the fixed-window root against pow, both codecs against pyref, the refusals of tests/bytes_cases.py, and the
endomorphism test of the r-torsion against g2_in_subgroup and against [r] Q in Python on 29 points of the twist."""
import ctypes as C
import os
import random
import re
import subprocess
import numpy as np
import pytest
import pyref as P
import pk_raw
import verify_cases as V
import bytes_cases as BC
import keyfile_cases as K
from helpers import fp_arr, fp_vals, g1_arr, g2_arr, g1_pts, g2_pts
from gpu_common import load_binding, ROOT

p, r = P.Q_MOD, P.R_MOD
PKG = os.path.join(ROOT, "gnark-whir_amd")
HEADER = os.path.join(ROOT, "include", "mi355x_groth16_keyfile.h")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(K.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_keyfile.so")))


@pytest.fixture(scope="module")
def streams():
    """one toy key (nc = 200, two Pedersen keys) in both encodings"""
    cs, pk, dom, keys = K.toy(n_ped=2)
    return cs, pk, keys, {e: K.write_pk_stream(pk, keys, e) for e in (K.RAW, K.COMPRESSED)}


# ---------------------------------------------------------------------------------------------------- the ABI
def test_library_exports_every_keyfile_symbol():
    B = load_binding()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))
    assert "mi_pk_load_stream" in names and "mi_groth16_setup_to_stream" in names
    for n in names:
        assert hasattr(B.load(), n), f"{n} declared in mi355x_groth16_keyfile.h but not exported"
    assert sorted(B.KEYFILE_EXPORTS) == names
    assert not set(B.KEYFILE_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) | set(B.VERIFY_BYTES_EXPORTS))
    assert C.sizeof(B.PedersenArrays) == 24 and C.sizeof(B.KeyfileStats) == 20
    flags = dict(re.findall(r"#define (MI_KEYFILE_[A-Z_]+) (\d+)u", open(HEADER).read()))
    assert (int(flags["MI_KEYFILE_RAW"]), int(flags["MI_KEYFILE_COMPRESSED"])) == (B.KEYFILE_RAW, B.KEYFILE_COMPRESSED) == (K.RAW, K.COMPRESSED)
    assert (int(flags["MI_KEYFILE_NO_SUBGROUP_CHECK"]), int(flags["MI_KEYFILE_SUBGROUP_BY_R"])) == (B.KEYFILE_NO_SUBGROUP_CHECK, B.KEYFILE_SUBGROUP_BY_R)


# ---------------------------------------------------------------------------------------------------- the inspector
@pytest.mark.parametrize("encoding", [K.RAW, K.COMPRESSED])
def test_stream_inspect_counts_and_offsets(streams, encoding):
    B = load_binding()
    cs, pk, keys, blobs = streams
    blob = blobs[encoding]
    g1, g2 = (32, 64) if encoding == K.COMPRESSED else (64, 128)
    info, enc = B.pk_stream_inspect(blob)
    assert enc == encoding
    assert info.log_n == pk["log_n"] and info.nb_wires == cs.nb_wires and info.n_commitment_keys == 2
    assert (info.n_g1_a, info.n_g1_b, info.n_g1_k, info.n_g1_z, info.n_g2_b) == tuple(len(pk[k]) for k in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"))
    assert info.off_alpha1 == 8 + 5 * 32 + 1 and info.off_g1_a == info.off_alpha1 + 3 * g1 + 4
    assert info.off_g1_b == info.off_g1_a + g1 * info.n_g1_a + 4 and info.off_g1_z == info.off_g1_b + g1 * info.n_g1_b + 4
    assert info.off_g1_k == info.off_g1_z + g1 * info.n_g1_z + 4 and info.off_beta2 == info.off_g1_k + g1 * info.n_g1_k
    assert info.off_g2_b == info.off_beta2 + 2 * g2 + 4
    assert blob[info.off_g1_a:info.off_g1_a + g1] == K.g1_enc(pk["g1_a"][0], encoding)
    assert blob[info.off_g1_k + g1 * (info.n_g1_k - 1):info.off_g1_k + g1 * info.n_g1_k] == K.g1_enc(pk["g1_k"][-1], encoding)
    assert blob[info.off_g2_b:info.off_g2_b + g2] == K.g2_enc(pk["g2_b"][0], encoding)
    assert list(info.n_basis[:2]) == [7, 8]
    assert blob[info.off_basis_exp_sigma[1]:info.off_basis_exp_sigma[1] + g1] == K.g1_enc(keys[1][1][0], encoding)
    assert info.off_basis_exp_sigma[1] + g1 * 8 == len(blob)
    sizes = {k: getattr(info, k) for k in ("nb_wires", "n_g1_a", "n_g1_b", "n_g1_k", "n_g1_z", "n_g2_b")}
    assert B.pk_stream_size(sizes, [7, 8], encoding) == len(blob)


def test_stream_inspect_equals_raw_inspect_on_raw_streams(streams):
    B = load_binding()
    for n_ped in (0, 2):
        cs, pk, dom, keys = K.toy(nc=33, npub=33, seed=5, n_ped=n_ped)
        blob = pk_raw.write_pk_raw(pk, keys)
        info, enc = B.pk_stream_inspect(blob)
        assert enc == K.RAW and bytes(info) == bytes(B.pk_raw_inspect(blob))
    # the compressed stream of the same key is no raw stream, and half the point bytes
    comp = K.write_pk_stream(pk, keys, K.COMPRESSED)
    with pytest.raises(B.MiError):
        B.pk_raw_inspect(comp)
    head = 8 + 5 * 32 + 1
    assert len(blob) - len(comp) == sum(32 * len(pk[k]) for k in ("g1_a", "g1_b", "g1_k", "g1_z")) + 64 * len(pk["g2_b"]) + 3 * 32 + 2 * 64 + 2 * 32 * (7 + 8) and head < len(comp)


@pytest.mark.parametrize("encoding", [K.RAW, K.COMPRESSED])
def test_stream_inspect_refusals(streams, encoding):
    B = load_binding()
    blob = streams[3][encoding]
    info, _ = B.pk_stream_inspect(blob)
    for bad in (blob[:-1], blob + b"\x00", blob[:100], b"", blob[:info.off_g1_z], blob + blob[-32:]):   # truncated, padded
        with pytest.raises(B.MiError):
            B.pk_stream_inspect(bad)
    for off in (info.off_g1_a - 1, info.off_g1_z - 1, info.off_g2_b - 1, info.off_basis[0] - 1):       # a count off by one
        broken = bytearray(blob); broken[off] ^= 1
        with pytest.raises(B.MiError):
            B.pk_stream_inspect(bytes(broken))
    broken = bytearray(blob); broken[7] = 3                                                              # cardinality not a power of two
    with pytest.raises(B.MiError):
        B.pk_stream_inspect(bytes(broken))
    # the section sizes say one encoding and the first point's flag bits the other
    broken = bytearray(blob); broken[info.off_alpha1] = (broken[info.off_alpha1] & 0x3F) | (0x80 if encoding == K.RAW else 0x00)
    with pytest.raises(B.MiError):
        B.pk_stream_inspect(bytes(broken))


def test_mutated_streams_never_trip_a_sanitizer(streams, tmp_path):
    """tests/cpp/keyfile_fuzz.cpp, its own main, -fsanitize=address,undefined on the host: mi_pk_stream_inspect over every truncation and
    seeded mutants of both encodings, each in a heap block of exactly its size; its contract checks run inside the program"""
    subprocess.check_call(["make", "-C", PKG, "-s", "sanitize-keyfile"])
    cs, pk, dom, keys = K.toy(nc=60, npub=4, seed=31, n_ped=2)
    paths = []
    for e in (K.RAW, K.COMPRESSED):
        paths.append(str(tmp_path / f"pk_{e}.bin"))
        open(paths[-1], "wb").write(K.write_pk_stream(pk, keys, e))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(PKG, "build", "keyfile_fuzz_asan"), paths[0], paths[1], "40000", "3"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    accepted, refused = (int(x) for x in res.stdout.split()[-2:])
    assert accepted > 50 and refused > 1000


# ---------------------------------------------------------------------------------------------------- the per-point text
def test_fixed_window_root_against_pow(emu):
    """the inputs of test_decode_cpu.test_fp_square_root_against_pow: the windowed chain gives pow(a, (p + 1) // 4, p), as the bit-by-bit one"""
    rnd = random.Random(3)
    vals = [0, 1, 4, 3, p - 1] + [rnd.randrange(p) for _ in range(60)]
    vals += [v * v % p for v in vals[5:25]]
    A = fp_arr(vals); Y = np.zeros_like(A); Y2 = np.zeros_like(A)
    assert emu.emu_kf_fp_root(V.p_(Y), V.p_(Y2), V.p_(A), C.c_size_t(len(vals))) == 0
    assert fp_vals(Y) == [pow(a, (p + 1) // 4, p) for a in vals]
    assert np.array_equal(Y, Y2)


def test_fp2_root_by_the_window_is_total(emu):
    rnd = random.Random(4)
    non = [v for v in (rnd.randrange(1, p) for _ in range(40)) if not BC.fp_is_residue(v)][:4] + [3, p - 1]
    seeded = [(rnd.randrange(p), rnd.randrange(p)) for _ in range(24)]
    vals = [(0, 0), (4, 0), (1, 0)] + [(a, 0) for a in non] + [(0, a) for a in non[:3]] + seeded + [P.fp2_sqr(v) for v in seeded[:8]]
    A = fp_arr([c for v in vals for c in v]).reshape(-1, 8); Y = np.zeros_like(A); ok = np.zeros(len(vals), np.uint8)
    assert emu.emu_kf_fp2_sqrt(V.p_(Y), V.p_(A), C.c_size_t(len(vals)), V.p_(ok)) == 0
    assert 8 < int(ok.sum()) < len(vals)
    for a, row, k in zip(vals, Y, ok):
        assert bool(k) == BC.fp2_has_root(a), a
        if k:
            assert P.fp2_sqr(tuple(fp_vals(row.reshape(2, 4)))) == (a[0] % p, a[1] % p), a


def _decode(emu, encs, g2, encoding):
    n = len(encs)
    out = np.zeros((n, 16 if g2 else 8), np.uint64); bad = np.zeros(n, np.uint8)
    fn = emu.emu_kf_decode_g2 if g2 else emu.emu_kf_decode_g1
    assert fn(b"".join(encs), C.c_size_t(n), C.c_int(encoding), V.p_(out), V.p_(bad)) == 0
    return out, bad


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("encoding", [K.RAW, K.COMPRESSED])
def test_codecs_round_trip_against_pyref(emu, g2, encoding):
    """both flag values, infinity, and on G2 y.A1 = 0 of both signs and a point outside the r-torsion: encode == pyref, decode inverts it"""
    pts = K.codec_points(40, 5, g2) + [None, V.twist_point_outside_subgroup() if g2 else P.G1_GEN]
    arr = g2_arr(pts) if g2 else g1_arr(pts)
    want = [(K.g2_enc if g2 else K.g1_enc)(q, encoding) for q in pts]
    if encoding == K.COMPRESSED:
        assert {e[0] >> 6 for e in want} == {1, 2, 3}
    out = C.create_string_buffer(len(b"".join(want)))
    assert (emu.emu_kf_encode_g2 if g2 else emu.emu_kf_encode_g1)(V.p_(arr), C.c_size_t(len(pts)), C.c_int(encoding), out) == 0
    assert out.raw == b"".join(want)
    back, bad = _decode(emu, want, g2, encoding)
    assert not bad.any() and np.array_equal(back, arr)


def test_compressed_refusals_are_those_of_the_proof_decoders(emu):
    for g2, edges in ((False, BC.g1_edge_encodings()), (True, BC.g2_edge_encodings())):
        out, bad = _decode(emu, [e for _, e, _ in edges], g2, K.COMPRESSED)
        for (name, _, want), b, row in zip(edges, bad, out):
            assert bool(b) == want, name
            if want:
                assert not row.any(), name
    encs = BC.seeded_g1_encodings(64, 6)
    out, bad = _decode(emu, encs, False, K.COMPRESSED)
    for e, b, row in zip(encs, bad, out):
        pt, m = BC.g1_decode_ref(e)
        assert bool(b) == m and g1_pts(row) == [pt], e.hex()
    encs2 = BC.seeded_g2_encodings(48, 7)
    out2, bad2 = _decode(emu, encs2, True, K.COMPRESSED)
    assert 10 <= int(bad2.sum()) <= 38
    for e, b, row in zip(encs2, bad2, out2):
        x = (int.from_bytes(e[32:], "big"), int.from_bytes(bytes([e[0] & 0x3F]) + e[1:32], "big"))
        has = x[0] < p and x[1] < p and BC.fp2_has_root(P.fp2_add(P.fp2_mul(P.fp2_sqr(x), x), P.G2_B))
        assert bool(b) == (not has), e.hex()
        if has:
            (Q,) = g2_pts(row)
            assert P.g2_is_on_curve(Q) and Q[0] == x and P.g2_compress(Q) == e


def test_raw_refusals_change_one_thing_each(emu):
    g, q = P.g1_mul(P.G1_GEN, 77), P.g2_mul(P.G2_GEN, 77)
    ok1, ok2 = pk_raw.g1_raw(g), pk_raw.g2_raw(q)
    pb = p.to_bytes(32, "big")
    g1_cases = [("point", ok1, False), ("infinity", pk_raw.g1_raw(None), False), ("flag 10", bytes([ok1[0] | 0x80]) + ok1[1:], True),
                ("flag 11", bytes([ok1[0] | 0xC0]) + ok1[1:], True), ("infinity, stray bit in Y", bytes([0x40]) + bytes(62) + b"\1", True),
                ("off the curve", ok1[:63] + bytes([ok1[63] ^ 1]), True), ("X = p", pb + ok1[32:], True), ("Y = y + p", ok1[:32] + (g[1] + p).to_bytes(32, "big"), True),
                ("(0, 0) under flag 00", bytes(64), True)]
    g2_cases = [("point", ok2, False), ("infinity", pk_raw.g2_raw(None), False), ("flag 10", bytes([ok2[0] | 0x80]) + ok2[1:], True),
                ("infinity, stray bit in Y.A0", bytes([0x40]) + bytes(126) + b"\1", True), ("off the twist", ok2[:127] + bytes([ok2[127] ^ 1]), True),
                ("X.A0 = p", ok2[:32] + pb + ok2[64:], True), ("Y.A1 = p", ok2[:64] + pb + ok2[96:], True),
                ("on the twist, outside the r-torsion", pk_raw.g2_raw(V.twist_point_outside_subgroup()), False)]
    for g2, cases in ((False, g1_cases), (True, g2_cases)):
        out, bad = _decode(emu, [e for _, e, _ in cases], g2, K.RAW)
        for (name, _, want), b, row in zip(cases, bad, out):
            assert bool(b) == want, name
            if want:
                assert not row.any(), name
    assert (g[1] + p) < (1 << 256)


def test_endomorphism_test_agrees_with_r_times_q(emu):
    """29 points of the twist (keyfile_cases.subgroup_cases): the psi test == g2_in_subgroup == [r] Q is infinity in Python, and infinity"""
    cases = K.subgroup_cases()
    pts = g2_arr([q for _, q, _ in cases] + [None])
    by_psi = np.zeros(30, np.uint8); by_r = np.zeros(30, np.uint8)
    assert emu.emu_kf_subgroup(V.p_(pts), C.c_size_t(30), V.p_(by_psi), V.p_(by_r)) == 0
    for (name, _, want), a, b in zip(cases, by_psi, by_r):
        assert bool(a) == want and bool(b) == want, name
    assert by_psi[29] == 1 and by_r[29] == 1
