"""GPU: verify from files (include/mi355x_groth16_vkfile.h; csrc/vkfile.hip, csrc/verify_bytes.hip).  Every comparison is exact.

1  k_witness_decode through mi_debug_witness_decode_dev against Python, the bytes at an odd device address
2  mi_vk_load_stream on the four toy keys, both encodings, lists empty and not: the verdicts of a batch of nine through the three
   verify_bytes bodies equal those of the handle mi_vk_load + mi_vk_set_public_committed builds, and the reference's
3  load refusals: MI_EINVAL, the field named, the ledger unchanged
4  mi_vk_write against the writer in Python, byte for byte
5  Setup -> both streams -> a second context -> prove -> verify_files accepts
6  verify_files* equals verify_bytes* on batches of 1, 9 and 65
"""
import random
import struct
import numpy as np
import pytest
import pyref as P
import cref
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import bytes_cases as BC
import keyfile_cases as K
import vkfile_cases as VK
import setup_cases as S
import r1cs_cases as RC
import dlog_keys as D
from helpers import fr_arr, fr_vals, g1_arr, g1_pts, g2_arr
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
r = P.R_MOD
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- 1: the witness decoder
@pytest.mark.parametrize("n,n_pub", [(0, 4), (1, 1), (1, 63), (1, 64), (3, 65), (257, 1)])
def test_witness_decode_kernel_against_python(ctx, n, n_pub):
    rnd = random.Random(1000 * n + n_pub)
    vals = [[rnd.randrange(r) for _ in range(n_pub)] for _ in range(n)]
    edges = list(VK.WITNESS_EDGES)
    if (n, n_pub) == (1, 1):
        vals[0][0] = r - 1
    elif n == 1:
        vals[0][:3] = edges[:3]; vals[0][n_pub - 1] = r - 1                  # one row, good to its last lane
    elif n == 3:
        vals[0][:3] = edges[:3]; vals[1][64] = r; vals[2][0] = r + 1; vals[2][63] = (1 << 256) - 1   # rows good, bad, bad
    elif n == 257:
        for i, e in zip((0, 1, 63, 64, 65, 256), edges):                     # bad rows on both sides of a wave's edge, and the last
            vals[i][0] = e
    flat = [v for row in vals for v in row]
    want_bad = [int(any(v >= r for v in row)) for row in vals]
    want = fr_arr([v if v < r else 0 for v in flat]).reshape(n, n_pub, 4) if n else np.zeros((0, n_pub, 4), np.uint64)
    if n > 1:
        assert 0 < sum(want_bad) < n
    for odd in (True, False):   # an odd address (byte loads), and an aligned one as a batch's staging image has it (16-byte loads)
        got, bad = ctx.witness_decode_dev(b"".join(v.to_bytes(32, "big") for v in flat), n, n_pub, odd=odd)
        assert list(bad) == want_bad and np.array_equal(got, want), odd
    if n:
        assert [sum(int(w) << (64 * i) for i, w in enumerate(got[0, 0]))] == [VK.mont(flat[0]) if flat[0] < r else 0]


# ---------------------------------------------------------------------------------------------------- 2: the loader
@pytest.fixture(scope="module")
def nine():
    """{shape: (case, lists, the batch of nine with the reference's verdicts)}: the pairings in Python run once"""
    out = {}
    for shape in VK.KEY_SHAPES:
        case, lists = VK.toy_key(*shape)
        if shape == (5, 1):   # one key with K[1] at infinity
            case = VK.with_k1_at_infinity(case)
        out[shape] = (case, lists, VK.batch_of_nine(case, lists))
    return out


def _bytes_items(items):
    return [(b, fr_arr(pub) if pub else None) for _, b, pub, _ in items]


@pytest.mark.parametrize("shape", VK.KEY_SHAPES)
@pytest.mark.parametrize("encoding", [VK.RAW, VK.COMPRESSED])
def test_loaded_key_judges_as_the_key_from_points(ctx, nine, shape, encoding):
    B = load_binding()
    case, lists, items = nine[shape]
    want = [v for *_, v in items]
    vk = case["vk"]
    d, nbp, ped = V.vk_arrays(vk)
    for ls in ([[] for _ in lists], lists) if shape[1] else (lists,):
        blob = VK.write_vk_stream(vk, vk["ped"], ls, encoding)
        a = ctx.vk_load(d, nbp, ped)
        b = ctx.vk_load_stream(blob)
        try:
            a.set_public_committed(ls)
            assert (b.nb_public, b.n_commitments) == (a.nb_public, a.n_commitments) == shape
            batch = _bytes_items(items)
            got_a, got_b = list(a.verify_bytes_batch(batch)), list(b.verify_bytes_batch(batch))
            assert got_a == got_b
            if ls == lists:
                assert got_b == want, [(n, g, w) for (n, *_), g, w in zip(items, got_b, want) if g != w]
            assert a.verify_bytes_combined(batch, SEED) == b.verify_bytes_combined(batch, SEED) == (R.MALFORMED, 3)
            clean = [batch[0], batch[6], batch[8]]
            assert a.verify_bytes_combined(clean, SEED) == b.verify_bytes_combined(clean, SEED)
            if ls == lists:
                assert b.verify_bytes_combined(clean, SEED) == (R.OK, 3)
            (va, sa), (vb, sb) = a.verify_bytes_locate(batch, SEED), b.verify_bytes_locate(batch, SEED)
            assert list(va) == list(vb) == got_b and sa == sb
        finally:
            a.free(); b.free()


# ---------------------------------------------------------------------------------------------------- 3: load refusals
def _refusal_streams():
    """name -> (stream, flags, the words the message must hold)"""
    B = load_binding()
    case, lists = VK.toy_key(3, 2)
    vk, ped = case["vk"], case["vk"]["ped"]
    comp = VK.write_vk_stream(vk, ped, lists, VK.COMPRESSED)
    raw = VK.write_vk_stream(vk, ped, lists, VK.RAW)
    ci, _ = B.vk_stream_inspect(comp)
    ri, _ = B.vk_stream_inspect(raw)
    no_y = next(e for name, e, _ in BC.g1_edge_encodings() if name == "X without y")
    plant = lambda blob, off, enc: blob[:off] + enc + blob[off + len(enc):]
    outside = V.twist_point_outside_subgroup()
    other_g = P.g2_mul(P.G2_GEN, 2)
    k3 = ri.off_k + 64 * 3
    return {
        "K[2] has an x without y": (plant(comp, ci.off_k + 64, no_y), 0, ["G1.K[2]"]),
        "K[3] and K[1] both bad": (plant(plant(comp, ci.off_k + 96, no_y), ci.off_k + 32, no_y), 0, ["G1.K[1]"]),
        "gamma outside the r-torsion": (VK.write_vk_stream(dict(vk, gamma2=outside), ped, lists, VK.COMPRESSED), 0, ["G2.Gamma", "r-torsion"]),
        "delta at infinity": (VK.write_vk_stream(dict(vk, delta2=None), ped, lists, VK.COMPRESSED), 0, ["G2.Delta", "infinity"]),
        "delta at infinity, unchecked": (VK.write_vk_stream(dict(vk, delta2=None), ped, lists, VK.COMPRESSED), B.KEYFILE_NO_SUBGROUP_CHECK, ["G2.Delta", "infinity"]),
        "two Pedersen keys with different G": (VK.write_vk_stream(vk, [ped[0], (other_g, ped[1][1])], lists, VK.COMPRESSED), 0, ["CommitmentKeys[1].G", "share one G"]),
        "GSigmaNeg outside the r-torsion": (VK.write_vk_stream(vk, [ped[0], (ped[1][0], outside)], lists, VK.RAW), 0, ["CommitmentKeys[1].GSigmaNeg", "r-torsion"]),
        "raw K off the curve": (raw[:k3 + 63] + bytes([raw[k3 + 63] ^ 1]) + raw[k3 + 64:], 0, ["G1.K[3]", "raw"]),
        "raw G1.Delta not below p": (plant(raw, ri.off_delta1, P.Q_MOD.to_bytes(32, "big")), 0, ["G1.Delta"]),
        "the layout": (comp[:-1], 0, ["CommitmentKeys"]),
    }


@pytest.mark.parametrize("name", ["K[2] has an x without y", "K[3] and K[1] both bad", "gamma outside the r-torsion", "delta at infinity",
                                  "delta at infinity, unchecked", "two Pedersen keys with different G", "GSigmaNeg outside the r-torsion",
                                  "raw K off the curve", "raw G1.Delta not below p", "the layout"])
def test_load_stream_refusals(ctx, name):
    B = load_binding()
    blob, flags, words = _refusal_streams()[name]
    ctx.trim()
    before = ctx.mem_ledger()
    with pytest.raises(B.MiError) as ei:
        ctx.vk_load_stream(blob, flags)
    msg = str(ei.value)
    assert ("rc=-1" in msg or "mi_vk_stream_inspect" in msg) and all(w in msg for w in words), msg
    assert ctx.mem_ledger() == before


def test_unchecked_load_takes_a_gamma_outside_the_subgroup(ctx):
    """MI_KEYFILE_NO_SUBGROUP_CHECK is gnark's UnsafeReadFrom: the membership test alone is skipped, the stream still has to decode"""
    B = load_binding()
    case, lists = VK.toy_key(3, 2)
    vk = dict(case["vk"], gamma2=V.twist_point_outside_subgroup())
    blob = VK.write_vk_stream(vk, vk["ped"], lists, VK.COMPRESSED)
    h = ctx.vk_load_stream(blob, B.KEYFILE_NO_SUBGROUP_CHECK)
    h.free()
    for flags in (0, B.KEYFILE_SUBGROUP_BY_R):
        with pytest.raises(B.MiError, match=r"G2\.Gamma.*r-torsion"):
            ctx.vk_load_stream(blob, flags)


# ---------------------------------------------------------------------------------------------------- 4: the writer
def _vk_dict(vk):
    d, nbp, ped = V.vk_arrays(vk)
    d.update(beta1=g1_arr([vk["beta1"]])[0], delta1=g1_arr([vk["delta1"]])[0])
    return d, nbp, ped


@pytest.mark.parametrize("shape", VK.KEY_SHAPES)
@pytest.mark.parametrize("encoding", [VK.RAW, VK.COMPRESSED])
def test_vk_write_against_python(ctx, shape, encoding):
    B = load_binding()
    case, lists = VK.toy_key(*shape)
    vk = case["vk"]
    if shape == (33, 0):
        vk = dict(vk, k=vk["k"][:5] + [None] + vk["k"][6:])      # an infinity among K
    d, nbp, ped = _vk_dict(vk)
    want = VK.write_vk_stream(vk, vk["ped"], lists, encoding)
    assert ctx.vk_write(d, nbp, ped, lists, encoding) == want and ctx.keyfile_len == len(want)
    assert ctx.vk_write(d, nbp, ped, None, encoding) == VK.write_vk_stream(vk, vk["ped"], None, encoding)
    with pytest.raises(B.MiError, match=str(len(want))):          # one byte short: the size comes back, nothing is written
        ctx.vk_write(d, nbp, ped, lists, encoding, cap=len(want) - 1)
    assert ctx.keyfile_len == len(want) and not any(ctx.keyfile_out)
    if shape[1]:
        with pytest.raises(B.MiError, match="pc_indices"):
            ctx.vk_write(d, nbp, ped, [[nbp]] + [[] for _ in lists[1:]], encoding)
    h = ctx.vk_load_stream(want)                                   # and what was written loads
    h.free()


def test_vk_write_leaves_the_buffer_alone_when_the_device_step_fails(ctx):
    """mi_debug_inject_hip_failure walks the checked HIP calls of mi_vk_write (a call returns an error code; nothing faults): each
    failure is MI_EHIP with out_host untouched, and the next write is right"""
    B = load_binding()
    case, lists = VK.toy_key(3, 2)
    d, nbp, ped = _vk_dict(case["vk"])
    want = VK.write_vk_stream(case["vk"], case["vk"]["ped"], lists, VK.COMPRESSED)
    failed = 0
    try:
        for nth in range(1, 9):
            assert ctx.lib.mi_debug_inject_hip_failure(nth) == 0
            try:
                got = ctx.vk_write(d, nbp, ped, lists, VK.COMPRESSED)
                assert got == want                                 # past the last checked call: the failure did not fire in this call
                break
            except B.MiError as e:
                failed += 1
                assert "rc=-2" in str(e) and not any(ctx.keyfile_out), nth
            finally:
                ctx.lib.mi_debug_inject_hip_failure(0)
    finally:
        ctx.lib.mi_debug_inject_hip_failure(0)
    assert failed >= 5
    assert ctx.vk_write(d, nbp, ped, lists, VK.COMPRESSED) == want


# ---------------------------------------------------------------------------------------------------- 5: Setup -> streams -> load -> prove -> verify
def test_setup_to_streams_round_trip(ctx):
    """the recipe of tests/test_gpu_verify_bytes.py::made with one commitment (the value of the commitment wire IS the hash of the
    commitment), the keys taken from the two streams in a second context"""
    B = load_binding()
    nc, n, nab, nb_public = 1, 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 41, long_lens=(16, 17, 64), commitments=nc, n_committed=7)
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 42)
    td = S.synth_trapdoor(51, n_sigma=nc)
    rr, ss = cref.gen_scalars(2, 61, 0)
    pk_blob, vk_blob, pkh, peds, vk = ctx.setup_to_streams(r1cs, td, K.COMPRESSED)
    ctx2 = B.Context(0)
    pool = B.Prover(0, 1)
    try:
        assert (len(pk_blob), len(vk_blob)) == (ctx.keyfile_len, ctx.vkfile_len)
        # the verifying key's stream is the Python writer's over what mi_groth16_setup returns and mi_pedersen_vk_make computes
        ped_vk = ctx.pedersen_vk_make(np.stack(td["sigma"]))
        from helpers import g2_pts
        pts = {n_: g2_pts(vk[n_].reshape(1, 16))[0] for n_ in ("beta2", "gamma2", "delta2")}
        tdi = {n_: D._int(td[n_]) for n_ in ("beta", "delta")}
        pyvk = dict(pts, alpha1=g1_pts(vk["alpha1"].reshape(1, 8))[0], beta1=P.g1_mul(P.G1_GEN, tdi["beta"]), delta1=P.g1_mul(P.G1_GEN, tdi["delta"]),
                    k=g1_pts(vk["k"]))
        pyped = [tuple(g2_pts(ped_vk[k])) for k in range(nc)]
        assert vk_blob == VK.write_vk_stream(pyvk, pyped, None, K.COMPRESSED)
        # the proving key's stream is mi_groth16_setup_to_stream's
        only, _, _, _ = ctx.setup_to_stream(r1cs, td, K.COMPRESSED, build=False)
        assert only == pk_blob
        # too small a room for either stream: refused with both sizes, before any point is computed
        for caps in (dict(cap=len(pk_blob) - 1), dict(vk_cap=len(vk_blob) - 1)):
            with pytest.raises(B.MiError, match="takes"):
                ctx.setup_to_streams(r1cs, td, K.COMPRESSED, build=False, **caps)
            assert (ctx.keyfile_len, ctx.vkfile_len) == (len(pk_blob), len(vk_blob))
        # a second context loads both
        removed = sorted(int(x) for ws, cw in r1cs["commitments"] for x in list(ws) + [cw])
        pkh2, peds2 = ctx2.pk_load_stream(pk_blob, nb_public, removed)
        vkh = ctx2.vk_load_stream(vk_blob)
        try:
            pub = fr_vals(W[1:nb_public])
            vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
            cms = np.stack([pool.commit(peds2[k], vals[k]).reshape(8) for k in range(nc)])
            values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
            for (_, cw), v in zip(r1cs["commitments"], values):
                W[cw] = fr_arr([v])[0]
            a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
            W[nab:] = D._op(2, a, b)
            proof, _ = pool.wait(pool.submit_bsb22(pkh2, W, a, b, None, rr, ss, [(peds2[k], vals[k]) for k in range(nc)], fr_arr([fold])[0]))
            data = B.proof_write(proof["raw"], commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8))
            wit = B.public_witness_write(np.ascontiguousarray(W[1:nb_public]))
            assert wit == VK.write_witness(pub)
            assert vkh.verify_files(data, wit) == B.VERIFY_OK
            assert vkh.verify_files(data, VK.write_witness([(pub[0] + 1) % r] + pub[1:])) == B.VERIFY_PAIRING
        finally:
            vkh.free()
            for pd in peds2:
                ctx2.pedersen_pk_free(pd)
            ctx2.pk_free(pkh2)
    finally:
        pool.close()
        ctx2.close()
        for pd in peds:
            ctx.pedersen_pk_free(pd)
        ctx.pk_free(pkh)


# ---------------------------------------------------------------------------------------------------- 6: verify_files* == verify_bytes*
NOT_REDUCED = np.array([[int((r >> (64 * i)) & ((1 << 64) - 1)) for i in range(4)]], np.uint64)   # the word string of r: not below r


@pytest.fixture(scope="module")
def forged():
    """per key: (forge key, 12 accepted proofs for the hashes as (proof bytes, public inputs))"""
    out = {}
    for shape in ((1, 0), (33, 1)):
        key = F.forge_key(*shape)
        honest = []
        for i in range(12):
            c = BC.hashed_honest(key, 900 + i)
            assert F.verdict_in_exponent(key, c) == R.OK
            honest.append((BC.proof_bytes_of(c), list(c["pub"])))
        out[shape] = (key, honest)
    return out


def _batch(key, honest, n):
    """[(proof bytes for verify_files, witness bytes, proof bytes for verify_bytes, the public inputs verify_bytes gets)] of n proofs;
    beside honest ones, from index 1 on (n >= 9): Krs tampered, pok tampered, a point that does not decode, one changed public input,
    a witness with a value equal to r, a header count off by one, a full witness with secrets appended, a header whose counts do not
    add up.  Where the WITNESS alone is at fault (6 and 8) verify_files gets the honest proof's bytes, so its verdict 3 can only come
    from the witness's header, and verify_bytes gets a proof with a broken count as a malformed stand-in."""
    n_pub, nc = key["nb_public"] - 1, key["n_commitments"]
    arr = lambda pub: fr_arr(pub) if pub else None
    out = []
    for i in range(n):
        b, pub = honest[i % len(honest)]
        w, pw = VK.write_witness(pub), arr(pub)
        bb = None                                                              # verify_bytes' proof, where it is not verify_files'
        flip = lambda at: b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]          # the other y of the point at this offset
        if n >= 9:
            if i == 1:
                b = flip(96)
            elif i == 2 and nc:
                b = flip(132 + 32 * nc)
            elif i == 3:
                b = bytes([b[0] & 0x3F]) + b[1:]
            elif i == 4 and n_pub:
                other = [(pub[0] + 1) % r] + pub[1:]
                w, pw = VK.write_witness(other), arr(other)
            elif i == 5 and n_pub:
                bad = n_pub - 1 if n == 9 else 0
                w = w[:12 + 32 * bad] + r.to_bytes(32, "big") + w[12 + 32 * bad + 32:]
                pw = pw.copy(); pw[bad] = NOT_REDUCED[0]
            elif i == 6:
                w = struct.pack(">III", n_pub + 1, 0, n_pub + 1) + w[12:] + bytes(32)
                bb = b[:128] + (nc + 1).to_bytes(4, "big") + b[132:]
            elif i == 7:
                w = VK.write_witness(pub, n_secret=2 + i)
            elif i == 8:
                w = struct.pack(">III", n_pub, 1, n_pub) + w[12:]              # nbPublic is the key's, the length is the header's n: the sum is not
                bb = b[:128] + (nc + 1).to_bytes(4, "big") + b[132:]
        out.append((b, w, b if bb is None else bb, pw))
    return out


@pytest.mark.parametrize("shape", [(1, 0), (33, 1)])
@pytest.mark.parametrize("n", [1, 9, 65])
def test_verify_files_equals_verify_bytes(ctx, forged, shape, n):
    B = load_binding()
    key, honest = forged[shape]
    d, nbp, ped = V.vk_arrays(key["vk"])
    vkh = ctx.vk_load(d, nbp, ped)
    try:
        if shape[1]:
            vkh.set_public_committed([[] for _ in range(shape[1])])
        batch = _batch(key, honest, n)
        files = [(b, w) for b, w, _, _ in batch]
        byts = [(bb, pw) for _, _, bb, pw in batch]
        assert all(f[0] == honest[i % len(honest)][0] for i, f in enumerate(files) if i in (6, 8) or n == 1)
        want = list(vkh.verify_bytes_batch(byts))
        got = list(vkh.verify_files_batch(files))
        assert got == want
        if n >= 9:
            n_pub = shape[0] - 1
            assert want[:9] == [0, 1, 2 if shape[1] else 0, 3, 1 if n_pub else 0, 3 if n_pub else 0, 3, 0, 3] and not any(want[9:])
        else:
            assert want == [0] and vkh.verify_files(*files[0]) == 0
        assert vkh.verify_files_combined(files, SEED) == vkh.verify_bytes_combined(byts, SEED)
        ok = [i for i, v in enumerate(want) if v == 0]
        for subset in (ok, ok + [1]) if n >= 9 else (ok,):
            got_c = vkh.verify_files_combined([files[i] for i in subset], SEED)
            assert got_c == vkh.verify_bytes_combined([byts[i] for i in subset], SEED) and got_c[0] == (0 if subset == ok else 1)
        (vf, sf), (vb, sb) = vkh.verify_files_locate(files, SEED), vkh.verify_bytes_locate(byts, SEED)
        assert list(vf) == list(vb) == want and sf == sb
        # the header against the key and against itself, one proof at a time under the HONEST proof's bytes: every witness below has
        # the length its own third count states, so each is a verdict, and the verdict comes from the header alone
        hb, hpub = honest[0]
        hw = VK.write_witness(hpub)
        n_pub = shape[0] - 1
        assert vkh.verify_files(hb, hw) == 0 and vkh.verify_files(hb, VK.write_witness(hpub, n_secret=1)) == 0
        heads = [(n_pub + 1, 0, n_pub + 1, bytes(32)), (n_pub, 1, n_pub, b""), (n_pub, 0, n_pub + 1, bytes(32)), (n_pub + 1, 0, n_pub, b"")]
        if n_pub:   # one value fewer is public: the last public input would be a SECRET value passed off as one; and no public part at all
            heads += [(n_pub - 1, 1, n_pub, b""), (0, n_pub, n_pub, b""), (n_pub - 1, 0, n_pub - 1, None)]
        for w_pub, w_sec, w_n, tail in heads:
            body = hw[12:] + tail if tail is not None else hw[12:-32]
            assert len(body) == 32 * w_n
            assert vkh.verify_files(hb, struct.pack(">III", w_pub, w_sec, w_n) + body) == 3, (w_pub, w_sec, w_n)
        # framing: a witness_len that is not 12 + 32 n of the witness's own header is the caller's error, and no verdict is written
        for wrong in (files[-1][1] + b"\0", files[-1][1][:-1], files[-1][1][:11], files[-1][1] + bytes(32)):
            out = np.full(n, 255, np.uint8)
            with pytest.raises(B.MiError, match="witness_len"):
                vkh.verify_files_batch(files[:-1] + [(files[-1][0], wrong)], out)
            assert set(out) == {255}
        with pytest.raises(B.MiError, match="proof_len"):
            vkh.verify_files_batch([(files[0][0] + b"\0", files[0][1])])
    finally:
        vkh.free()
