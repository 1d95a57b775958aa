"""GPU suite: groth16.Verify from a proof's bytes (include/mi355x_groth16_verify_bytes.h) -- the decode and hash kernels through their
debug entry points against the host build of the same text (tests/emu/emu_decode.cpp) and hashlib, Setup / Prove / mi_proof_write /
verify-from-bytes round trips whose commitment values and challenge are the hashes, the forged cases of tests/verify_forge.py that have
an encoding (verdict from the exponent rule with those hashes), byte-level refusals, batches against the per-proof calls, framing."""
import ctypes as C
import random
import numpy as np
import pytest
import pyref as P
import cref
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import bytes_cases as BC
import setup_cases as S
import r1cs_cases as RC
import dlog_keys as D
from helpers import fr_arr, fr_vals, g1_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
r = P.R_MOD
LANES = [1, 63, 64, 65, 130]

# the cases of verify_forge.cases() that cannot be written as bytes: a coordinate that is not reduced, a point off its curve
NO_ENCODING = [
    "2pub_0com: Ar off the curve", "2pub_0com: Krs off the curve", "2pub_0com: Bs off the twist", "2pub_0com: Ar off the curve and Krs + 1",
    "3pub_3com: Ar off the curve", "3pub_3com: Krs off the curve", "3pub_3com: Bs off the twist", "3pub_3com: Ar off the curve and Krs + 1",
    "3pub_3com: pok off the curve", "3pub_3com: C_2 off the curve", "3pub_3com: Ar.x + p", "3pub_3com: Ar.y + p", "3pub_3com: Bs.x.a1 + p",
    "3pub_3com: Bs.y.a0 + p", "3pub_3com: Krs.y + p", "3pub_3com: pok.x + p", "3pub_3com: C_1.y + p", "3pub_3com: Ar.x = 2^256 - 1",
    "3pub_3com: pok.y = p", "3pub_3com: Ar = (p, p)", "3pub_3com: Bs = (p, p, p, p)", "2pub_0com: Krs.x + p", "3pub_1com: C_0.x + p"]


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(BC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_decode.so")))


# ---------------------------------------------------------------------------------------------------- device against the host build
@pytest.mark.parametrize("n", LANES)
def test_decode_kernels_equal_the_host_build(ctx, emu, n):
    """a single lane, the wave edges, a partial last wave behind a full one: points and flags word for word"""
    for g2, edges, seeded in ((False, BC.g1_edge_encodings(), BC.seeded_g1_encodings), (True, BC.g2_edge_encodings(), BC.seeded_g2_encodings)):
        encs = [e for _, e, _ in edges]
        encs = [encs[3]] if n == 1 else (encs + seeded(n, 100 + n))[:n]
        w = 16 if g2 else 8
        want = np.zeros((n, w), np.uint64); wbad = np.zeros(n, np.uint8)
        (emu.emu_decode_g2 if g2 else emu.emu_decode_g1)(b"".join(encs), C.c_size_t(n), V.p_(want), V.p_(wbad))
        got, bad = ctx.decode_points(b"".join(encs), g2=g2)
        assert np.array_equal(bad, wbad) and np.array_equal(got, want), g2
        if n > 1:
            assert list(bad[:len(edges)]) == [int(m) for _, _, m in edges][:n]
            assert 0 < int(bad.sum()) < n


@pytest.mark.parametrize("n", [1, 65])
def test_hash_kernel_equals_hashlib(ctx, n):
    rnd = random.Random(n)
    for ln in BC.SHA_LENGTHS:
        for dst in (BC.DST_COMMITMENT, rnd.randbytes(255)) if ln in (0, 64, 119) else (BC.DST_FOLD,):
            msgs = [rnd.randbytes(ln) for _ in range(n)]
            assert fr_vals(ctx.hash_to_field_dev(dst, msgs)) == [BC.hash_to_field(m, dst) for m in msgs], (ln, len(dst))
    lib = ctx.lib
    buf = ctx.alloc(64)
    try:
        assert lib.mi_debug_hash_to_field_dev(ctx.h, C.c_void_p(buf.ptr), C.c_uint32(0), C.c_void_p(buf.ptr), C.c_size_t(1), C.c_size_t(1), C.c_void_p(buf.ptr)) == -1
        assert lib.mi_debug_hash_to_field_dev(ctx.h, C.c_void_p(buf.ptr), C.c_uint32(256), C.c_void_p(buf.ptr), C.c_size_t(1), C.c_size_t(1), C.c_void_p(buf.ptr)) == -1
        assert lib.mi_debug_decode_g1_dev(ctx.h, None, C.c_size_t(1), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr)) == -1
        assert lib.mi_debug_decode_g2_dev(ctx.h, C.c_void_p(buf.ptr), C.c_size_t(1), None, C.c_void_p(buf.ptr)) == -1
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------------- Setup, Prove, write, verify from bytes
@pytest.fixture(scope="module", params=[0, 1, 2])
def made(ctx, request):
    """the recipe of tests/test_gpu_verify.py::made on a 2^10 domain, with two differences: the commitments are listed by ascending
    commitment wire (value i then multiplies K[nb_public + i], as the bytes path defines it), and the value of commitment wire i IS the
    hash of commitment i -- computed here in Python, written into W before the rest of the witness is solved -- and the challenge the
    prover folds with is the hash of those values."""
    B = load_binding()
    nc = request.param
    n, nab, nb_public = 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 40 + nc, long_lens=(16, 17, 64), commitments=nc, n_committed=7)
    r1cs["commitments"] = sorted(r1cs["commitments"], key=lambda c: c[1])
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 41 + nc)
    td = S.synth_trapdoor(50 + nc, n_sigma=nc)
    rr, ss = cref.gen_scalars(2, 60 + nc, 0)
    pkh, peds, vk = ctx.setup(r1cs, td)
    pub = fr_vals(W[1:nb_public])
    pool = B.Prover(0, 1) if nc else None
    try:
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]      # committed wires are never commitment wires
        cms = np.stack([pool.commit(peds[k], vals[k]).reshape(8) for k in range(nc)]) if nc else np.zeros((0, 8), np.uint64)
        values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
        for (_, cw), v in zip(r1cs["commitments"], values):
            W[cw] = fr_arr([v])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        if nc:
            proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, rr, ss, [(peds[k], vals[k]) for k in range(nc)], fr_arr([fold])[0]))
        else:
            rh = ctx.r1cs_load(r1cs)
            proof, _ = ctx.prove_w(pkh, rh, W, rr, ss)
            ctx.r1cs_free(rh)
    finally:
        if pool:
            pool.close()
    inp = {"raw": proof["raw"].copy(), "public_inputs": np.ascontiguousarray(W[1:nb_public])}
    ped_vk = None
    if nc:
        ped_vk = ctx.pedersen_vk_make(np.stack(td["sigma"]))
        inp.update(commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8), fold_challenge=fr_arr([fold])[0], commitment_values=fr_arr(values))
    vkh = ctx.vk_load(vk, nb_public, ped_vk)
    data = B.proof_write(inp["raw"], commitments=cms if nc else None, pok=inp.get("pok"))
    yield dict(nc=nc, vkh=vkh, inp=inp, data=data, pub=inp["public_inputs"])
    vkh.free()
    for pd in peds:
        ctx.pedersen_pk_free(pd)
    ctx.pk_free(pkh)


def test_setup_prove_write_verify_bytes_accepts(made):
    B = load_binding()
    vkh, data, pub, nc = made["vkh"], made["data"], made["pub"], made["nc"]
    assert len(data) == 164 + 32 * nc
    assert vkh.verify(made["inp"]) == B.VERIFY_OK              # the struct path, given the Python hashes
    assert vkh.verify_bytes(data, pub) == B.VERIFY_OK
    other = pub.copy(); other[0] = fr_arr([D._int(other[0]) + 1])[0]
    assert vkh.verify_bytes(data, other) == B.VERIFY_PAIRING
    flipped = bytes([data[0] ^ 0x40]) + data[1:]
    assert vkh.verify_bytes(flipped, pub) == B.VERIFY_PAIRING
    assert vkh.verify_bytes(data[:128] + (nc + 1).to_bytes(4, "big") + data[132:], pub) == B.VERIFY_MALFORMED
    if nc:
        i = 132 + 32 * nc                                        # -pok
        assert vkh.verify_bytes(data[:i] + bytes([data[i] ^ 0x40]) + data[i + 1:], pub) == B.VERIFY_PEDERSEN
        vkh.set_public_committed([[1]] + [[] for _ in range(nc - 1)])   # the prover hashed with empty lists: other values now
        assert vkh.verify_bytes(data, pub) == B.VERIFY_PAIRING
        vkh.set_public_committed([[] for _ in range(nc)])
        assert vkh.verify_bytes(data, pub) == B.VERIFY_OK


# ---------------------------------------------------------------------------------------------------- forged cases
@pytest.fixture(scope="module")
def forged_vk(ctx):
    loaded = {}

    def get(key):
        if key["id"] not in loaded:
            d, nbp, ped = V.vk_arrays(key["vk"])
            loaded[key["id"]] = ctx.vk_load(d, nbp, ped)
        return loaded[key["id"]]
    yield get
    for h in loaded.values():
        h.free()


def _pub(case):
    return fr_arr(case["pub"]) if case["pub"] else None


def test_the_excluded_cases_are_those_without_an_encoding():
    cases = F.cases()
    assert [c["name"] for c in cases if BC.has_no_encoding(c)] == NO_ENCODING
    assert len(NO_ENCODING) <= sum(1 for c in cases if c["words"] or c["malformed"]) == 33
    assert all(c["want"] == R.MALFORMED for c in cases if c["name"] in NO_ENCODING)


@pytest.mark.parametrize("key_id", F.CASE_KEY_IDS)
def test_forged_cases_get_the_verdict_of_the_exponent_with_hashed_values(forged_vk, key_id):
    """every case of this key that has an encoding, in ONE batch: its commitment values and challenge are the hashes of its commitments
    now, so the verdict is the exponent rule's for those; a non-reduced public input stays malformed"""
    mine = [c for c in F.cases() if c["key"]["id"] == key_id and c["name"] not in NO_ENCODING]
    assert mine
    key = mine[0]["key"]
    vkh = forged_vk(key)
    seen = [BC.rehashed(c) for c in mine]
    want = [F.verdict_in_exponent(key, c) for c in seen]
    items = []
    for c in seen:
        pub = F.verify_input(c).get("public_inputs") if c["pub"] else None     # carries the words that are not reduced
        items.append((BC.proof_bytes_of(c), pub))
    got = list(vkh.verify_bytes_batch(items))
    assert got == want, [(c["name"], g, w) for c, g, w in zip(mine, got, want) if g != w]
    if key["n_commitments"] == 0:
        assert R.OK in want                                      # nothing to hash: the accepted cases stay accepted
    for k, seed in enumerate((700, 701)):                        # and accepted proofs FOR the hashes
        c = BC.hashed_honest(key, seed + key["n_commitments"])
        assert F.verdict_in_exponent(key, c) == R.OK and vkh.verify_bytes(BC.proof_bytes_of(c), _pub(c)) == R.OK


def test_byte_level_refusals(forged_vk):
    key = F.forge_key(3, 3)
    vkh = forged_vk(key)
    c = BC.hashed_honest(key, 710)
    data = BC.proof_bytes_of(c)
    items, names = [(data, _pub(c))], ["accepted"]
    for name, enc, bad in BC.g1_edge_encodings():
        if bad:
            for what, off in (("Ar", 0), ("Krs", 96), ("C_1", 164), ("pok", 228)):
                items.append((data[:off] + enc + data[off + 32:], _pub(c))); names.append(f"{what}: {name}")
    for name, enc, bad in BC.g2_edge_encodings():
        if bad:
            items.append((data[:32] + enc + data[96:], _pub(c))); names.append(f"Bs: {name}")
    outside = P.g2_compress(V.twist_point_outside_subgroup())   # decodes, and is then refused by the r-torsion check
    items.append((data[:32] + outside + data[96:], _pub(c))); names.append("Bs outside the r-torsion")
    got = list(vkh.verify_bytes_batch(items))
    assert got == [R.OK] + [R.MALFORMED] * (len(items) - 1), [n for n, g in zip(names, got) if g != R.MALFORMED]
    assert len(items) > 40


@pytest.mark.parametrize("shape,lists", [((3, 1), None), ((3, 3), [[], [1, 3], [2]])])
def test_batch_of_distinct_proofs_equals_the_per_proof_calls(ctx, forged_vk, shape, lists):
    """70 accepted proofs with their own inputs, then one byte broken at 0, 63, 64 and 69 and the proof of 30 under the inputs of 31:
    every entry is judged on its own bytes, a malformed one leaves its neighbours alone; a second identical batch allocates nothing"""
    key = F.forge_key(*shape)
    nc = shape[1]
    vkh = forged_vk(key)
    if lists:
        vkh.set_public_committed(lists)
    try:
        batch = BC.hashed_distinct_batch(key, 70, 800 + nc, lists)
        assert all(v == R.OK for _, _, v in batch) and len({b for b, _, _ in batch}) == 70
        def broken(i, off, mask, verdict):
            b = batch[i][0]
            batch[i][0] = b[:off] + bytes([b[off] ^ mask]) + b[off + 1:]
            batch[i][2] = verdict
        broken(0, 31, 0xFF, None)                    # Ar's X changed: malformed or another point, the decoder's reference says which
        batch[0][2] = R.MALFORMED if BC.g1_decode_ref(batch[0][0][:32])[1] else R.PAIRING
        broken(63, 0, 0x40, R.PAIRING)               # -Ar
        broken(64, 132 + 32 * nc, 0x40, R.PEDERSEN)  # -pok
        broken(69, 131, 0x01, R.MALFORMED)           # the count
        batch[31] = [batch[30][0], batch[31][1], R.PAIRING]
        items = [(b, fr_arr(pub)) for b, pub, _ in batch]
        want = [v for _, _, v in batch]
        got = list(vkh.verify_bytes_batch(items))
        assert got == want
        before = ctx.mem_ledger()
        assert list(vkh.verify_bytes_batch(items)) == want
        assert ctx.mem_ledger() == before
        assert [vkh.verify_bytes(b, pub) for b, pub in items] == want
        for n in (1, 3):
            assert list(vkh.verify_bytes_batch(items[62:62 + n])) == want[62:62 + n]
        assert len(vkh.verify_bytes_batch([])) == 0
    finally:
        if lists:
            vkh.set_public_committed([[] for _ in range(nc)])


# ---------------------------------------------------------------------------------------------------- framing and lifetime
def test_framing_errors_and_the_lifetime_of_the_lists(ctx):
    B = load_binding()
    key = F.forge_key(3, 3)
    d, nbp, ped = V.vk_arrays(key["vk"])
    vkh = ctx.vk_load(d, nbp, ped)
    c = BC.hashed_honest(key, 900)
    data, pub = BC.proof_bytes_of(c), fr_arr(c["pub"])
    assert vkh.verify_bytes(data, pub) == B.VERIFY_OK
    for bad in (data[:-1], data + b"\0", data[:164], b""):
        with pytest.raises(B.MiError, match="proof_len"):
            vkh.verify_bytes(bad, pub)
    with pytest.raises(B.MiError, match="public_inputs"):
        vkh.verify_bytes(data, None)
    v = C.c_uint8()
    lib = ctx.lib
    assert lib.mi_groth16_verify_bytes(ctx.h, vkh.h, None, C.c_size_t(len(data)), V.p_(pub), C.byref(v)) == -1
    assert lib.mi_groth16_verify_bytes(ctx.h, vkh.h, data, C.c_size_t(len(data)), V.p_(pub), None) == -1
    assert lib.mi_groth16_verify_bytes(ctx.h, None, data, C.c_size_t(len(data)), V.p_(pub), C.byref(v)) == -1
    assert lib.mi_groth16_verify_bytes_batch(ctx.h, vkh.h, None, C.c_size_t(2), C.byref(v)) == -1
    # only the public wires and EARLIER commitments may be committed: j in 1 .. nb_public - 1 + i
    for lists, what in (([[3], [], []], r"indices\[0\] = 3 of commitment 0"), ([[], [1, 4], []], r"indices\[1\] = 4 of commitment 1"),
                        ([[], [], [0]], r"indices\[0\] = 0 of commitment 2"), ([[], [], [5]], r"indices\[0\] = 5 of commitment 2")):
        with pytest.raises(B.MiError, match=what):
            vkh.set_public_committed(lists)
    off = np.array([0, 2, 1, 1], np.uint32)
    assert lib.mi_vk_set_public_committed(ctx.h, vkh.h, V.p_(off), V.p_(np.array([1, 1], np.uint32))) == -1 and b"offsets[2]" in lib.mi_last_error(ctx.h)
    assert lib.mi_vk_set_public_committed(ctx.h, vkh.h, None, None) == -1
    assert vkh.verify_bytes(data, pub) == B.VERIFY_OK            # a refused list changed nothing
    vkh.set_public_committed([[2], [1, 3], [2, 4, 3]])
    assert vkh.verify_bytes(data, pub) == B.VERIFY_PAIRING
    before = ctx.mem_ledger()
    vkh.free()                                                    # the lists are host memory of the key: nothing stays on the device
    vkh2 = ctx.vk_load(d, nbp, ped)
    assert vkh2.verify_bytes(data, pub) == B.VERIFY_OK            # a fresh key starts with empty lists
    vkh2.free()
    assert ctx.mem_ledger() == before
