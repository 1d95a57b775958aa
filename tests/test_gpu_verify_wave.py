"""GPU suite: the verifier with one wave per pairing (include/mi355x_groth16_verify_wave.h; csrc/verify_wave.hip over fp12_wave.cuh and
pairing_wave.cuh).  Every Fp result is fully reduced, so the wave's order of evaluation must give the words of the one-lane kernels: the
two debug entry points against theirs word for word, whole proofs from mi_groth16_setup keys and from bytes against
mi_groth16_verify_batch / mi_groth16_verify_bytes_batch byte for byte, the forged, edge and non-reduced cases of tests/verify_forge.py
against the verdict computed in the exponent, and the two bodies alternating on one context, whose workspace they share."""
import ctypes as C
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
from helpers import fr_arr, g1_arr, g2_arr
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- the debug entry points
@pytest.mark.parametrize("n", [1, 2, 5])
def test_pairing_equals_the_one_lane_kernels(ctx, n):
    """the grid is n workgroups: one, two, and a few; infinity in G1 at the first and in G2 at the last index"""
    ps, qs = V.seeded_pairs(n, 2000 + n)
    pa, qa = g1_arr(ps), g2_arr(qs)
    for final in (False, True):
        got = ctx.pairing_wave(pa, qa, final_exp=final)
        assert np.array_equal(got, ctx.pairing(pa, qa, final_exp=final)), f"final_exp={final}"
    one = V.gt_arr([R.to_tower(R.ONE)])[0]
    assert np.array_equal(got[0], one) and (n == 1 or np.array_equal(got[-1], one))
    assert n < 3 or not np.array_equal(got[1], one)
    if n < 3:      # with infinity at both ends nothing of these sizes ran a Miller loop: the same sizes over finite points
        ps, qs = V.seeded_pairs(n, 2100 + n, inf_first_last=False)
        pa, qa = g1_arr(ps), g2_arr(qs)
        for final in (False, True):
            got = ctx.pairing_wave(pa, qa, final_exp=final)
            assert np.array_equal(got, ctx.pairing(pa, qa, final_exp=final)) and not np.array_equal(got[0], one), f"final_exp={final}"


def test_more_items_than_the_grid_has_workgroups(ctx):
    """a grid is capped at 4096 workgroups (MI_WAVE_GRID_CAP, csrc/verify_wave.hip), which walk their items with the grid's stride:
    4096 + 3 records and pairs, so the first three workgroups take a second item and the rest do not"""
    n = 4096 + 3
    rng = np.random.default_rng(4099)
    words = rng.integers(0, 1 << 62, (n, 12, 4), dtype=np.uint64); words[:, :, 3] >>= 2      # every Fp word string below 2^252 < p
    X = words.reshape(n, 48); Y = np.ascontiguousarray(X[::-1])
    assert np.array_equal(ctx.fp12_op_wave(V.F12_MUL, X, Y), ctx.fp12_op(V.F12_MUL, X, Y))
    ps, qs = V.seeded_pairs(n, 4100)
    pa, qa = g1_arr(ps), g2_arr(qs)
    assert np.array_equal(ctx.pairing_wave(pa, qa, final_exp=False), ctx.pairing(pa, qa, final_exp=False))


@pytest.mark.parametrize("n", [1, 3])
def test_fp12_ops_equal_the_one_lane_kernel(ctx, n):
    """every op code on all-zero, one, all p - 1 (n = 3) and on a seeded value (n = 1)"""
    rng = np.random.default_rng(177 + n)
    xs = [[0] * 12, [1] + [0] * 11, [R.p - 1] * 12] if n == 3 else [[int.from_bytes(rng.bytes(31), "little") for _ in range(12)]]
    X = V.gt_arr(xs); Y = np.ascontiguousarray(X[::-1])
    for op in range(V.F12_OP_END):
        assert np.array_equal(ctx.fp12_op_wave(op, X, Y), ctx.fp12_op(op, X, Y)), op
    for op in (V.F12_SQR, V.F12_CONJ, V.F12_FINAL_EXP):
        assert np.array_equal(ctx.fp12_op_wave(op, X), ctx.fp12_op(op, X)), op      # y_dev = NULL
    E = ctx.fp12_op(V.F12_EASY, X)
    assert np.array_equal(ctx.fp12_op_wave(V.F12_CYCLO_SQR, E), ctx.fp12_op(V.F12_SQR, E))


def test_debug_entry_points_refuse_what_the_one_lane_ones_refuse(ctx):
    lib = ctx.lib
    buf = ctx.to_dev(V.gt_arr([[1] + [0] * 11]))
    try:
        for bad in (-1, V.F12_OP_END):
            assert lib.mi_debug_fp12_op_wave_dev(ctx.h, C.c_int(bad), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
        assert lib.mi_debug_fp12_op_wave_dev(ctx.h, C.c_int(0), None, C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
        assert lib.mi_debug_fp12_op_wave_dev(ctx.h, C.c_int(0), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), None, C.c_size_t((1 << 24) + 1)) != 0
        assert lib.mi_debug_pairing_wave_dev(ctx.h, None, None, C.c_size_t(1), C.c_void_p(buf.ptr), C.c_uint32(0)) != 0
        assert lib.mi_debug_pairing_wave_dev(ctx.h, C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t(1), C.c_void_p(buf.ptr), C.c_uint32(2)) != 0
        assert lib.mi_debug_pairing_wave_dev(None, C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t(1), C.c_void_p(buf.ptr), C.c_uint32(0)) != 0
        assert lib.mi_debug_pairing_wave_dev(ctx.h, None, None, C.c_size_t(0), None, C.c_uint32(0)) == 0      # no pair, no launch
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------------- whole proofs
def _small_solved(nc_commit, seed):
    """a solvable skewed R1CS of 600 constraints (tests/r1cs_cases.py: rows of C are single wires that take (A W)(B W)) -- the system
    of tests/test_gpu_verify.py's `made` fixture"""
    n, nab, nb_public = 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, seed, long_lens=(16, 17, 64), commitments=nc_commit, n_committed=7)
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, seed + 1)
    a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
    W[nab:] = D._op(2, a, b)
    return r1cs, W, a, b


@pytest.fixture(scope="module", params=[0, 1, 2])
def made(ctx, request):
    """key by mi_groth16_setup under a forgotten trapdoor, Pedersen vk by mi_pedersen_vk_make, proof by mi_groth16_prove_w (no
    commitment) or mi_prover_submit_bsb22, the verifying key loaded"""
    B = load_binding()
    nc = request.param
    r1cs, W, a, b = _small_solved(nc, 40 + nc)
    td = S.synth_trapdoor(50 + nc, n_sigma=nc)
    r, s = cref.gen_scalars(2, 60 + nc, 0)
    pkh, peds, vk = ctx.setup(r1cs, td)
    nb_public = r1cs["nb_public"]
    inp = {"public_inputs": np.ascontiguousarray(W[1:nb_public])}
    if nc == 0:
        rh = ctx.r1cs_load(r1cs)
        proof, _ = ctx.prove_w(pkh, rh, W, r, s)
        ctx.r1cs_free(rh)
        ped_vk = None
    else:
        ch = cref.gen_scalars(1, 70, 0)[0]
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
        pool = B.Prover(0, 1)
        try:
            cms = np.stack([pool.commit(peds[k], vals[k]).reshape(8) for k in range(nc)])
            proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, r, s, [(peds[k], vals[k]) for k in range(nc)], ch))
        finally:
            pool.close()
        ped_vk = ctx.pedersen_vk_make(np.stack(td["sigma"]))
        inp.update(commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8), fold_challenge=ch,
                   commitment_values=np.ascontiguousarray(W[sorted(cw for _, cw in r1cs["commitments"])]))
    inp["raw"] = proof["raw"].copy()
    vkh = ctx.vk_load(vk, nb_public, ped_vk)
    yield dict(nc=nc, vkh=vkh, inp=inp)
    vkh.free()
    for pd in peds:
        ctx.pedersen_pk_free(pd)
    ctx.pk_free(pkh)


def _tampers(made):
    """one tamper per verdict code: 1 (another Krs), 2 (another pok; without commitments the second equation does not exist), 3 twice
    (Bs outside the r-torsion: the psi test must say what [r] Bs says; Ar off the curve: the host's answer)"""
    B = load_binding()
    inp = made["inp"]

    def with_raw(lo, hi, val):
        x = inp["raw"].copy(); x[lo:hi] = val
        return dict(inp, raw=x)

    out = [(with_raw(24, 32, g1_arr([P.g1_mul(P.G1_GEN, 1009)])[0]), B.VERIFY_PAIRING),
           (with_raw(8, 24, g2_arr([V.twist_point_outside_subgroup()])[0]), B.VERIFY_MALFORMED),
           (with_raw(0, 8, g1_arr([(1, 3)])[0]), B.VERIFY_MALFORMED)]
    if made["nc"]:
        out.append((dict(inp, pok=g1_arr([P.g1_mul(P.G1_GEN, 1003)])[0]), B.VERIFY_PEDERSEN))
    return out


def test_setup_prove_verify_wave_accepts_and_names_each_tamper(made):
    B = load_binding()
    vkh = made["vkh"]
    assert list(vkh.verify_wave([made["inp"]])) == [B.VERIFY_OK]
    for x, want in _tampers(made):
        assert list(vkh.verify_wave([x])) == [want] == list(vkh.verify_batch([x]))
    assert len(vkh.verify_wave([])) == 0


def test_batch_of_seven_equals_the_batch_call_byte_for_byte(made):
    """tampered proofs at the first, a middle and the last index"""
    vkh = made["vkh"]
    t = _tampers(made)
    proofs = [made["inp"]] * 7
    proofs[0], proofs[3], proofs[6] = t[1][0], t[-1][0], t[0][0]
    want = vkh.verify_batch(proofs)
    assert list(want) == [t[1][1], 0, 0, t[-1][1], 0, 0, t[0][1]]
    assert np.array_equal(vkh.verify_wave(proofs), want)


def test_the_two_bodies_alternate_on_one_context(made):
    """WS_VERIFY is shared: after a call of the old body on the same context, and the other way round, the verdicts are unchanged;
    the batches shrink and grow between the calls"""
    vkh = made["vkh"]
    t = _tampers(made)
    big = [made["inp"], t[0][0], t[1][0]] * 3
    small = [t[-1][0], made["inp"]]
    want_big, want_small = vkh.verify_batch(big), vkh.verify_batch(small)
    assert np.array_equal(vkh.verify_wave(big), want_big)
    assert np.array_equal(vkh.verify_batch(small), want_small)
    assert np.array_equal(vkh.verify_wave(small), want_small)
    assert np.array_equal(vkh.verify_batch(big), want_big)
    assert np.array_equal(vkh.verify_wave(big), want_big)
    out, ms = vkh.verify_wave_split(small)
    assert np.array_equal(out, want_small) and set(ms) == set(load_binding().VERIFY_WAVE_SPLIT_PHASES) and all(v >= 0 for v in ms.values())
    print("\nsplit of a call of 2 proofs, ms:", {k: round(v, 3) for k, v in ms.items()})


# ---------------------------------------------------------------------------------------------------- from bytes
def test_from_bytes_equals_the_bytes_batch_call(ctx):
    """3 proofs, one of them with a flipped byte"""
    key = F.forge_key(3, 1)
    d, nbp, ped = V.vk_arrays(key["vk"])
    vkh = ctx.vk_load(d, nbp, ped)
    try:
        cs = [BC.hashed_honest(key, 910 + i) for i in range(3)]
        items = [(BC.proof_bytes_of(c), fr_arr(c["pub"])) for c in cs]
        data = bytearray(items[1][0]); data[100] ^= 0x10                     # inside Krs.x
        items[1] = (bytes(data), items[1][1])
        want = vkh.verify_bytes_batch(items)
        assert want[0] == want[2] == R.OK and want[1] != R.OK
        assert np.array_equal(vkh.verify_bytes_wave(items), want)
        assert len(vkh.verify_bytes_wave([])) == 0
    finally:
        vkh.free()


# ---------------------------------------------------------------------------------------------------- forged, edge and non-reduced inputs
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


@pytest.mark.parametrize("key_id", F.CASE_KEY_IDS)
def test_forged_cases_get_the_verdict_of_the_exponent_alone_and_as_one_batch(forged_vk, key_id):
    mine = [c for c in F.cases() if c["key"]["id"] == key_id]
    assert mine
    vkh = forged_vk(mine[0]["key"])
    want = [F.verdict_in_exponent(c["key"], c) for c in mine]
    assert want == [c["want"] for c in mine]
    inputs = [F.verify_input(c) for c in mine]
    got = list(vkh.verify_wave(inputs))
    assert got == want, [(c["name"], g, w) for c, g, w in zip(mine, got, want) if g != w]
    alone = [int(vkh.verify_wave([x])[0]) for x in inputs]
    assert alone == want, [(c["name"], g, w) for c, g, w in zip(mine, alone, want) if g != w]


def test_refusals_are_those_of_the_batch_call_under_the_prefix_of_this_one(ctx, forged_vk):
    key = F.forge_key(2, 2)
    vkh = forged_vk(key)
    lib = ctx.lib
    inp = F.verify_input(F.honest(key, 77))
    arr, keep = vkh._inputs([inp, inp])
    out = np.full(2, 255, np.uint8)
    vd = out.ctypes.data_as(C.c_void_p)

    def refused(message, vk, a, n, v):
        assert lib.mi_groth16_verify_wave(ctx.h, vk, a, C.c_size_t(n), v) == -1, message
        assert lib.mi_last_error(ctx.h).decode() == f"verify wave: {message}"
        assert out.tolist() == [255, 255], message

    refused("null vk, input or verdict pointer", None, arr, 2, vd)
    refused("null vk, input or verdict pointer", vkh.h, None, 2, vd)
    refused("more than 2^24 proofs in one batch", vkh.h, arr, (1 << 24) + 1, vd)
    refused("null vk, input or verdict pointer", vkh.h, arr, 2, None)
    cv_null = "commitments, pok or commitment_values is null"
    for name, message in (("commitments", cv_null), ("public_inputs", "public_inputs is null"), ("pok", cv_null),
                          ("fold_challenge", "fold_challenge is null with more than one commitment"), ("commitment_values", cv_null)):
        one_out, keep1 = vkh._inputs([inp, {k: x for k, x in inp.items() if k != name}])
        refused(message, vkh.h, one_out, 2, vd)
    assert lib.mi_groth16_verify_wave(None, vkh.h, arr, C.c_size_t(2), vd) == -1
    assert lib.mi_groth16_verify_wave(ctx.h, vkh.h, None, C.c_size_t(0), None) == 0
    assert lib.mi_groth16_verify_wave(ctx.h, vkh.h, arr, C.c_size_t(2), vd) == 0 and out.tolist() == [R.OK, R.OK]
