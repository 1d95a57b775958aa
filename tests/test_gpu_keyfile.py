"""GPU: proving keys as files (include/mi355x_groth16_keyfile.h, csrc/keyfile.hip).  Every comparison is exact.

1  the bulk point codecs against pyref word for word and byte for byte, at sizes around a wave and a workgroup, and the lowest bad index
2  mi_pk_load_stream on the three keys of tests/test_pk_raw.py, compressed and raw: the proof of the loaded key against the oracle's
3  mi_pk_write_dev against the two writers in Python, byte for byte
4  Setup -> stream -> a second context -> the same proof, accepted under the verifying key Setup returned
5  refusals: MI_EINVAL, the message names section and index, the memory ledger does not move
"""
import numpy as np
import pytest
import pyref as P
import cref
import pk_raw
import bytes_cases as BC
import keyfile_cases as K
import setup_cases as S
import verify_cases as V
from helpers import fr_arr, g1_arr, g2_arr, toy_pk_arrays
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- 1: bulk codecs
def _decompress(ctx, blob, n, g2, flags=0):
    """-> (rc, first_bad, the (n, 8 or 16) words written)"""
    w = 16 if g2 else 8
    src = ctx.to_dev(np.frombuffer(blob, np.uint8)); dst = ctx.alloc(max(8 * w * n, 32))
    try:
        rc, first = ctx.decompress_dev(src.ptr, n, dst.ptr, g2, flags)
        return rc, first, dst.download((n, w))
    finally:
        src.free(); dst.free()


def _compress(ctx, arr, g2, encoding):
    n = arr.shape[0]
    size = (64 if g2 else 32) * (1 if encoding == K.COMPRESSED else 2)
    src = ctx.to_dev(arr); dst = ctx.alloc(max(size * n, 32) + 1)
    try:
        ctx.compress_dev(src.ptr, n, dst.ptr + 1, g2, encoding)   # an odd address: the strings of a stream are not aligned
        return bytes(dst.download(size * n + 1, np.uint8)[1:])
    finally:
        src.free(); dst.free()


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_bulk_codecs_against_pyref(ctx, n, g2):
    B = load_binding()
    pts = K.codec_points(n, 100 + n, g2)
    want = g2_arr(pts) if g2 else g1_arr(pts)
    blob = b"".join(K.g2_enc(q, K.COMPRESSED) if g2 else K.g1_enc(q, K.COMPRESSED) for q in pts)
    if n >= 63:
        assert {e >> 6 for e in blob[::64 if g2 else 32]} == {1, 2, 3}
    rc, first, got = _decompress(ctx, blob, n, g2, B.KEYFILE_NO_SUBGROUP_CHECK if g2 else 0)
    assert rc == 0 and first == B.NO_BAD_INDEX and np.array_equal(got, want.reshape(got.shape))
    assert _compress(ctx, got, g2, K.COMPRESSED) == blob
    assert _compress(ctx, got, g2, K.RAW) == b"".join(K.g2_enc(q, K.RAW) if g2 else K.g1_enc(q, K.RAW) for q in pts)
    if g2:   # the membership test names the first point that is not in the r-torsion (the one with y.A1 = 0, if it is not), by both rules
        member = {q: P.g2_mul(q, P.R_MOD) is None for q in set(pts) if q is not None}
        outside = [i for i, q in enumerate(pts) if q is not None and not member[q]][:1]
        for flags in (0, B.KEYFILE_SUBGROUP_BY_R):
            rc, first, got2 = _decompress(ctx, blob, n, True, flags)
            assert (rc, first) == ((-1, outside[0]) if outside else (0, B.NO_BAD_INDEX))
            assert np.array_equal(got2, got)


@pytest.mark.parametrize("g2", [False, True])
def test_first_bad_is_the_lower_of_two(ctx, g2):
    B = load_binding()
    n, size = 1000, 64 if g2 else 32
    base = [(P.g2_mul if g2 else P.g1_mul)(P.G2_GEN if g2 else P.G1_GEN, k) for k in range(1, 12)]
    pts = [base[i % 11] for i in range(n)]
    encs = [K.g2_enc(q, K.COMPRESSED) if g2 else K.g1_enc(q, K.COMPRESSED) for q in pts]
    edges = {name: e for name, e, bad in (BC.g2_edge_encodings() if g2 else BC.g1_edge_encodings()) if bad}
    encs[700] = edges["flag 00"]
    encs[300] = edges["only A0 >= p" if g2 else "X without y"]
    rc, first, got = _decompress(ctx, b"".join(encs), n, g2)
    want = (g2_arr(pts) if g2 else g1_arr(pts)).copy(); want[[300, 700]] = 0
    assert rc == -1 and first == 300 and np.array_equal(got, want)
    assert "300" in ctx.lib.mi_last_error(ctx.h).decode()
    if g2:   # a point outside the r-torsion at a lower index still: it is the first, unless the membership test is switched off
        encs[100] = P.g2_compress(V.twist_point_outside_subgroup())
        assert _decompress(ctx, b"".join(encs), n, True)[:2] == (-1, 100)
        assert _decompress(ctx, b"".join(encs), n, True, B.KEYFILE_NO_SUBGROUP_CHECK)[:2] == (-1, 300)


# ---------------------------------------------------------------------------------------------------- 2: loading
@pytest.mark.parametrize("nc,npub,seed", [(200, 5, 31), (1000, 3, 77), (33, 33, 5)])
def test_load_stream_and_prove_vs_oracle(ctx, nc, npub, seed):
    B = load_binding()
    cs, pk, dom, keys = K.toy(nc, npub, seed, n_ped=1)
    w, a, b, c = cs.solve()
    r, s = 123456789 + seed, 987654321 + seed
    W, A_, B_, C_ = fr_arr(w), fr_arr(a), fr_arr(b), fr_arr(c)
    want = P.proof_bytes(P.toy_prove(cs, pk, dom, r, s, msm=P.msm_pippenger))
    pkh2 = ctx.pk_load(toy_pk_arrays(pk))
    again, _ = ctx.prove(pkh2, W, A_, B_, C_, fr_arr([r])[0], fr_arr([s])[0])
    ctx.pk_free(pkh2)
    assert B.proof_write(again["raw"]) == want
    basis, bes = keys[0]
    vals = cref.gen_scalars(len(basis), 9, 1)
    for encoding in (K.COMPRESSED, K.RAW):
        blob = K.write_pk_stream(pk, keys, encoding)
        pkh, peds = ctx.pk_load_stream(blob, cs.nb_public)
        try:
            got, _ = ctx.prove(pkh, W, A_, B_, C_, fr_arr([r])[0], fr_arr([s])[0])
            assert B.proof_write(got["raw"]) == want                    # P.toy_prove's bytes
            assert np.array_equal(got["raw"], again["raw"])             # and mi_pk_load's on the same arrays
            assert len(peds) == 1
            assert np.array_equal(ctx.pedersen_commit(peds[0], vals), cref.pedersen_msm(g1_arr(basis), vals))
            assert np.array_equal(ctx.pedersen_commit(peds[0], vals, knowledge=True), cref.pedersen_msm(g1_arr(bes), vals))
            st = ctx.keyfile_stats()
            assert st["total_ms"] > 0 and st["decode_ms"] > 0
        finally:
            for pd in peds:
                ctx.pedersen_pk_free(pd)
            ctx.pk_free(pkh)


# ---------------------------------------------------------------------------------------------------- 3: writing
def test_write_dev_equals_the_python_writers(ctx):
    B = load_binding()
    cs, pk, dom, keys = K.toy(200, 5, 31, n_ped=1)
    arrs = toy_pk_arrays(pk)
    bufs = {name: ctx.to_dev(arrs[name]) for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b")}
    ped_bufs = [ctx.to_dev(g1_arr(keys[0][0])), ctx.to_dev(g1_arr(keys[0][1]))]
    try:
        dev = dict(arrs, **{name: (bufs[name].ptr, arrs[name].shape[0]) for name in bufs})
        ped = [(ped_bufs[0].ptr, ped_bufs[1].ptr, len(keys[0][0]))]
        raw = ctx.pk_write_dev(dev, ped, K.RAW)
        assert raw == pk_raw.write_pk_raw(pk, keys)
        comp = ctx.pk_write_dev(dev, ped, K.COMPRESSED)
        assert comp == K.write_pk_stream(pk, keys, K.COMPRESSED)
        assert ctx.pk_write_dev(dev, [], K.COMPRESSED) == K.write_pk_stream(pk, [], K.COMPRESSED)
        with pytest.raises(B.MiError):                                   # one byte short: refused, and told how much it takes
            ctx.pk_write_dev(dev, ped, K.COMPRESSED, cap=len(comp) - 1)
        assert ctx.keyfile_len == len(comp)
        with pytest.raises(B.MiError):
            ctx.pk_write_dev(dev, ped, 2)
    finally:
        for d in list(bufs.values()) + ped_bufs:
            d.free()


# ---------------------------------------------------------------------------------------------------- 4: Setup -> stream -> load -> prove
@pytest.mark.parametrize("encoding", [K.COMPRESSED, K.RAW])
def test_setup_to_stream_round_trip(ctx, encoding):
    """mi_groth16_setup_to_stream under a seeded trapdoor of tests/setup_cases.py, on the solvable skewed system of tests/test_gpu_verify.py
    with one commitment (the synthetic systems of setup_cases.py have no witness, and the last check needs one): the key loaded from the
    stream in a SECOND context gives, for the same (W, r, s), the proof of the resident key, and mi_groth16_verify accepts it"""
    from test_gpu_verify import _small_solved
    B = load_binding()
    r1cs, W, a, b = _small_solved(1, 41)
    td = S.synth_trapdoor(51, n_sigma=1)
    r, s = cref.gen_scalars(2, 61, 0)
    nb_public = r1cs["nb_public"]
    blob, pkh, peds, vk = ctx.setup_to_stream(r1cs, td, encoding)
    assert len(blob) == ctx.keyfile_len and B.pk_stream_inspect(blob)[1] == encoding
    removed = sorted(int(x) for ws, cw in r1cs["commitments"] for x in list(ws) + [cw])
    ctx2 = B.Context(0)
    pool = B.Prover(0, 1)
    pkh2, peds2 = ctx2.pk_load_stream(blob, nb_public, removed)
    try:
        ch = cref.gen_scalars(1, 70, 0)[0]
        vals = np.ascontiguousarray(W[r1cs["commitments"][0][0]])
        proofs = []
        for key, ped in ((pkh, peds[0]), (pkh2, peds2[0])):
            cm = pool.commit(ped, vals).reshape(8)
            proof, _ = pool.wait(pool.submit_bsb22(key, W, a, b, None, r, s, [(ped, vals)], ch))
            proofs.append((cm, proof))
        (cm1, p1), (cm2, p2) = proofs
        assert np.array_equal(cm1, cm2) and np.array_equal(p1["raw"], p2["raw"]) and np.array_equal(p1["pok"], p2["pok"])
        vkh = ctx.vk_load(vk, nb_public, ctx.pedersen_vk_make(np.stack(td["sigma"])))
        try:
            inp = dict(raw=p2["raw"].copy(), public_inputs=np.ascontiguousarray(W[1:nb_public]), commitments=cm2.reshape(1, 8),
                       pok=np.ascontiguousarray(p2["pok"]).reshape(8), fold_challenge=ch,
                       commitment_values=np.ascontiguousarray(W[[r1cs["commitments"][0][1]]]))
            assert vkh.verify(inp) == B.VERIFY_OK
        finally:
            vkh.free()
        # write only: the same bytes, no key; a buffer one byte short is refused before any point is computed, with the size it takes
        only, none_h, none_p, vk2 = ctx.setup_to_stream(r1cs, td, encoding, build=False)
        assert only == blob and none_h is None and np.array_equal(vk2["k"], vk["k"])
        with pytest.raises(B.MiError):
            ctx.setup_to_stream(r1cs, td, encoding, cap=len(blob) - 1)
        assert ctx.keyfile_len == len(blob)
    finally:
        pool.close()
        ctx2.pedersen_pk_free(peds2[0]); ctx2.pk_free(pkh2); ctx2.close()
        ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh)


# ---------------------------------------------------------------------------------------------------- 5: refusals
def _planted():
    """the compressed stream of the key of test_pk_raw.py with one Pedersen key, and what to plant where: name -> (offset of the
    string, its bytes, the section and index the message must name)"""
    cs, pk, dom, keys = K.toy(200, 5, 31, n_ped=1)
    blob = K.write_pk_stream(pk, keys, K.COMPRESSED)
    info, _ = load_binding().pk_stream_inspect(blob)
    e1 = {name: e for name, e, bad in BC.g1_edge_encodings() if bad}
    assert info.n_g1_z == 256 and info.n_g1_a > 3 and info.n_g2_b > 5 and info.n_basis[0] > 2
    a0 = blob[info.off_g1_k:info.off_g1_k + 32]
    return cs, blob, info, {
        "an x with no y, beyond the first workgroup": (info.off_g1_z + 32 * 150, e1["X without y"], "G1.Z[150]"),
        "x >= p": (info.off_g1_a + 32 * 3, e1["X = p"], "G1.A[3]"),
        "flag 00": (info.off_g1_k, bytes([a0[0] & 0x3F]) + a0[1:], "G1.K[0]"),
        "infinity with a stray bit": (info.off_basis[0] + 32 * 2, e1["flag 01, stray bit in the last byte"], "Basis[0][2]"),
        "outside the r-torsion": (info.off_g2_b + 64 * 5, P.g2_compress(V.twist_point_outside_subgroup()), "G2.B[5]"),
    }


@pytest.mark.parametrize("case", ["an x with no y, beyond the first workgroup", "x >= p", "flag 00", "infinity with a stray bit", "outside the r-torsion"])
def test_load_stream_refusals(ctx, case):
    B = load_binding()
    cs, blob, info, plants = _planted()
    off, enc, where = plants[case]
    broken = blob[:off] + enc + blob[off + len(enc):]
    assert len(broken) == len(blob)
    ctx.trim()
    before = ctx.mem_ledger()
    with pytest.raises(B.MiError) as ei:
        ctx.pk_load_stream(broken, cs.nb_public)
    assert "rc=-1" in str(ei.value) and where in str(ei.value)
    assert ("r-torsion" in str(ei.value)) == (case == "outside the r-torsion")
    assert ctx.mem_ledger() == before
    if case == "outside the r-torsion":   # gnark's UnsafeReadFrom: that same stream loads
        pkh, peds = ctx.pk_load_stream(broken, cs.nb_public, flags=B.KEYFILE_NO_SUBGROUP_CHECK)
        ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh)
    if case.startswith("an x with no y"):  # a second bad string further on in the section: the lower index is the one named
        off2 = info.off_g1_z + 32 * 200
        with pytest.raises(B.MiError, match=r"G1\.Z\[150\]"):
            ctx.pk_load_stream(broken[:off2] + enc + broken[off2 + 32:], cs.nb_public)


def test_load_stream_checks_raw_points_too(ctx):
    """what mi_pk_load_raw lets through: a raw point that is not on its curve, a raw G2 point outside the r-torsion"""
    B = load_binding()
    cs, pk, dom, keys = K.toy(200, 5, 31, n_ped=1)
    blob = pk_raw.write_pk_raw(pk, keys)
    info = B.pk_raw_inspect(blob)
    off = info.off_g1_b + 64 * 1 + 63
    with pytest.raises(B.MiError, match=r"G1\.B\[1\]"):
        ctx.pk_load_stream(blob[:off] + bytes([blob[off] ^ 1]) + blob[off + 1:], cs.nb_public)
    off = info.off_beta2 + 128
    outside = blob[:off] + pk_raw.g2_raw(V.twist_point_outside_subgroup()) + blob[off + 128:]
    with pytest.raises(B.MiError, match=r"G2\.BetaDelta\[1\].*r-torsion"):
        ctx.pk_load_stream(outside, cs.nb_public)
    pkh, peds = ctx.pk_load_raw(outside, cs.nb_public)      # (the older entry point takes it as it is)
    ctx.pedersen_pk_free(peds[0]); ctx.pk_free(pkh)
