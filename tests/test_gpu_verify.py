"""GPU suite: groth16.Verify on the device (include/mi355x_groth16_verify.h) -- the pairing and the tower through the two debug entry
points against the host build of the same code (tests/emu/emu_pairing.cpp) and the definitional reference (tests/pairing_ref.py), whole
proofs from mi_groth16_setup keys under a random trapdoor and from toy keys with known discrete logs, one tamper per verdict code,
batches against the per-proof calls, and the forged, edge and non-reduced inputs of tests/verify_forge.py, alone and in batches of
distinct proofs, against the verdict computed in the exponent."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import setup_cases as S
import r1cs_cases as RC
import dlog_keys as D
from helpers import fr_arr, g1_arr, g2_arr, g1_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(V.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_pairing.so")))


def _emu_pair(emu, pa, qa, final):
    out = np.zeros((len(pa), 48), np.uint64)
    assert emu.emu_pairing(V.p_(pa), V.p_(qa), C.c_size_t(len(pa)), V.p_(out), C.c_uint(1 if final else 0)) == 0
    return out


# ---------------------------------------------------------------------------------------------------- pairing parity
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_pairing_equals_the_host_build_and_the_reference(ctx, emu, n):
    """a single lane, the wave edges, a partial last wave behind a full one; infinity in G1 at the first and in G2 at the last index"""
    ps, qs = V.seeded_pairs(n, 1000 + n)
    pa, qa = g1_arr(ps), g2_arr(qs)
    for final in (False, True):
        got = ctx.pairing(pa, qa, final_exp=final)
        assert np.array_equal(got, _emu_pair(emu, pa, qa, final)), f"final_exp={final}"
    one = V.gt_arr([R.to_tower(R.ONE)])[0]
    assert np.array_equal(got[0], one) and (n == 1 or np.array_equal(got[-1], one))
    pick = sorted(set(int(i) for i in np.random.default_rng(n).integers(0, n, 3)) | {0, n - 1})[:8]
    assert V.gt_vals(got[pick]) == [R.pairing_tower(ps[i], qs[i]) for i in pick]


@pytest.mark.parametrize("n", [1, 65])
def test_fp12_ops_equal_the_host_build_and_the_reference(ctx, emu, n):
    rng = np.random.default_rng(77 + n)
    edge = [[0] * 12, [1] + [0] * 11, [R.p - 1] * 12]
    xs = ([[int(v) for v in rng.integers(0, 1 << 62, 12)] for _ in range(n)] if n == 1 else
          edge + [[int.from_bytes(rng.bytes(31), "little") for _ in range(12)] for _ in range(n - 3)])
    X = V.gt_arr(xs); Y = np.ascontiguousarray(X[::-1])
    for op in range(V.F12_OP_END):
        if op == V.F12_CYCLO_SQR:
            continue
        want = np.zeros_like(X)
        assert emu.emu_fp12_op(C.c_int(op), V.p_(want), V.p_(X), V.p_(Y), C.c_size_t(n)) == 0
        assert np.array_equal(ctx.fp12_op(op, X, Y), want), op
    E = ctx.fp12_op(V.F12_EASY, X)
    assert np.array_equal(ctx.fp12_op(V.F12_CYCLO_SQR, E), ctx.fp12_op(V.F12_SQR, E))
    ft, tt = R.from_tower, R.to_tower
    k = min(n, 4)
    assert V.gt_vals(ctx.fp12_op(V.F12_MUL, X[:k], Y[:k])) == [tt(R.f_mul(ft(a), ft(b))) for a, b in zip(xs[:k], V.gt_vals(Y[:k]))]
    assert V.gt_vals(ctx.fp12_op(V.F12_FINAL_EXP, X[-1:])) == [tt(R.f_pow(ft(xs[-1]), R.D_PRIME))]
    lib = ctx.lib
    buf = ctx.to_dev(X)
    try:
        for bad in (-1, V.F12_OP_END):
            assert lib.mi_debug_fp12_op_dev(ctx.h, C.c_int(bad), C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
        assert lib.mi_debug_fp12_op_dev(ctx.h, C.c_int(0), None, C.c_void_p(buf.ptr), None, C.c_size_t(1)) != 0
        assert lib.mi_debug_pairing_dev(ctx.h, None, None, C.c_size_t(1), C.c_void_p(buf.ptr), C.c_uint32(0)) != 0
        assert lib.mi_debug_pairing_dev(ctx.h, C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), C.c_size_t(1), C.c_void_p(buf.ptr), C.c_uint32(2)) != 0
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------------- end to end
def _small_solved(nc_commit, seed):
    """a solvable skewed R1CS of 600 constraints (tests/r1cs_cases.py: rows of C are single wires that take (A W)(B W))"""
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
    """key by mi_groth16_setup under a random trapdoor, Pedersen vk by mi_pedersen_vk_make, proof by mi_groth16_prove_w (no commitment) or
    mi_prover_submit_bsb22, the verifying key loaded.  The commitment's "hash" is the value of its wire: the library is hash-free."""
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
        # commitment_values[k] goes with K[nb_public + k], and mi_groth16_setup orders those points by ascending wire index; the case
        # with two commitments has its commitment wires in descending order, so the two orders differ there
        inp.update(commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8), fold_challenge=ch,
                   commitment_values=np.ascontiguousarray(W[sorted(cw for _, cw in r1cs["commitments"])]))
    inp["raw"] = proof["raw"].copy()
    vkh = ctx.vk_load(vk, nb_public, ped_vk)
    yield dict(nc=nc, vk=vk, vkh=vkh, inp=inp, nb_public=nb_public, ped_vk=ped_vk)
    vkh.free()
    for pd in peds:
        ctx.pedersen_pk_free(pd)
    ctx.pk_free(pkh)


def test_setup_prove_verify_accepts(ctx, made):
    B = load_binding()
    assert made["vkh"].verify(made["inp"]) == B.VERIFY_OK
    if made["nc"]:
        g = made["ped_vk"]
        assert np.array_equal(g[:, 0], g2_arr([P.G2_GEN] * made["nc"]))


def _other_g1(k):
    return g1_arr([P.g1_mul(P.G1_GEN, 1000 + k)])[0]


def test_rejections_change_one_thing_each(ctx, made):
    B = load_binding()
    inp, vkh, nc = made["inp"], made["vkh"], made["nc"]
    raw = inp["raw"]

    def with_raw(lo, hi, val):
        x = raw.copy(); x[lo:hi] = val
        return dict(inp, raw=x)

    cases = [("Ar", with_raw(0, 8, _other_g1(1)), B.VERIFY_PAIRING),
             ("Bs", with_raw(8, 24, g2_arr([P.g2_mul(P.G2_GEN, 77)])[0]), B.VERIFY_PAIRING),
             ("Krs", with_raw(24, 32, _other_g1(2)), B.VERIFY_PAIRING),
             ("Ar off the curve", with_raw(0, 8, g1_arr([(1, 3)])[0]), B.VERIFY_MALFORMED),
             ("Bs outside the r-torsion", with_raw(8, 24, g2_arr([V.twist_point_outside_subgroup()])[0]), B.VERIFY_MALFORMED)]
    pub = inp["public_inputs"].copy(); pub[0] = fr_arr([D._int(pub[0]) + 1])[0]
    cases.append(("public input + 1", dict(inp, public_inputs=pub), B.VERIFY_PAIRING))
    if nc:
        cv = inp["commitment_values"].copy(); cv[nc - 1] = fr_arr([D._int(cv[nc - 1]) + 1])[0]
        cases.append(("commitment value", dict(inp, commitment_values=cv), B.VERIFY_PAIRING))
        cases.append(("pok", dict(inp, pok=_other_g1(3)), B.VERIFY_PEDERSEN))
    if nc == 2:
        # kSum adds the commitments up, so their order does not reach the pairing equation: the Pedersen one (sigma_k, c^k) catches it
        cases.append(("commitments swapped", dict(inp, commitments=np.ascontiguousarray(inp["commitments"][::-1])), B.VERIFY_PEDERSEN))
        cases.append(("fold challenge", dict(inp, fold_challenge=fr_arr([D._int(inp["fold_challenge"]) + 1])[0]), B.VERIFY_PEDERSEN))
    for name, x, want in cases:
        assert vkh.verify(x) == want, name
    assert vkh.verify(inp) == B.VERIFY_OK


def test_vk_load_refusals(ctx, made):
    B = load_binding()
    vk, nbp, ped = made["vk"], made["nb_public"], made["ped_vk"]
    with pytest.raises(B.MiError):
        ctx.vk_load(vk, nbp, ped, n_k=len(vk["k"]) - 1)
    with pytest.raises(B.MiError):
        ctx.vk_load(dict(vk, gamma2=g2_arr([V.twist_point_outside_subgroup()])[0]), nbp, ped)
    with pytest.raises(B.MiError):
        ctx.vk_load(dict(vk, alpha1=g1_arr([(1, 3)])[0]), nbp, ped)
    if made["nc"] == 2:
        bad = ped.copy(); bad[1, 0] = g2_arr([P.g2_mul(P.G2_GEN, 2)])[0]
        with pytest.raises(B.MiError, match="share one G"):
            ctx.vk_load(vk, nbp, bad)
    h = C.c_void_p()
    assert ctx.lib.mi_vk_load(ctx.h, None, C.byref(h)) == -1 and ctx.lib.mi_groth16_verify(ctx.h, made["vkh"].h, None, None) == -1


@pytest.mark.parametrize("n_commitments", [0, 1])
def test_toy_key_with_known_discrete_logs(ctx, n_commitments):
    """the same proof judged three ways: in the exponent (pyref.trapdoor_check), by the reference's pairings, by the device"""
    B = load_binding()
    case = V.toy_case(n_commitments)
    assert P.trapdoor_check(case["cs"], case["td"], case["exps"], case["toy_proof"], case["r"], case["s"])
    vkd, nbp, ped = V.vk_arrays(case["vk"])
    vkh = ctx.vk_load(vkd, nbp, ped)
    try:
        assert vkh.verify(V.proof_dict(case)) == V.ref_verdict(case) == B.VERIFY_OK
        ar, bs, krs = case["proof"]
        other = P.g1_mul(P.G1_GEN, 4242)
        assert not P.trapdoor_check(case["cs"], case["td"], case["exps"], dict(case["toy_proof"], krs=other), case["r"], case["s"])
        assert vkh.verify(V.proof_dict(case, proof=(ar, bs, other))) == B.VERIFY_PAIRING
        if n_commitments:
            assert np.array_equal(ctx.pedersen_vk_make(fr_arr(case["sigmas"])), ped)
    finally:
        vkh.free()


# ---------------------------------------------------------------------------------------------------- batches
def test_batches_equal_the_per_proof_calls(ctx, made):
    """n = 1, 3, 70 with tampered proofs at 0, 63, 64 and n - 1; the second and third batch grow the workspace the first one made"""
    B = load_binding()
    inp, vkh = made["inp"], made["vkh"]
    x = inp["raw"].copy(); x[24:32] = _other_g1(9)
    bad_pairing = dict(inp, raw=x)
    y = inp["raw"].copy(); y[0:8] = g1_arr([(1, 3)])[0]
    bad_curve = dict(inp, raw=y)
    single = {id(inp): vkh.verify(inp), id(bad_pairing): vkh.verify(bad_pairing), id(bad_curve): vkh.verify(bad_curve)}
    assert sorted(single.values()) == [B.VERIFY_OK, B.VERIFY_PAIRING, B.VERIFY_MALFORMED]
    for n in (3, 1, 70, 3):
        proofs = [inp] * n
        for k, i in enumerate(sorted({0, 63, 64, n - 1})):
            if i < n:
                proofs[i] = (bad_pairing, bad_curve)[k % 2]
        got = vkh.verify_batch(proofs)
        assert list(got) == [single[id(pr)] for pr in proofs], n
    assert len(vkh.verify_batch([])) == 0


# ---------------------------------------------------------------------------------------------------- forged, edge and non-reduced inputs
@pytest.fixture(scope="module")
def forged_vk(ctx):
    """key of tests/verify_forge.py -> its mi_vk, loaded once"""
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
def test_forged_cases_get_the_verdict_of_the_exponent(forged_vk, key_id):
    """every case of verify_forge.cases() for this key: accepted edge proofs (kSum at infinity, the doubling and the cancelling branch of
    the group law, infinite K, Krs, C_k and pok, every fold power), each with one exponent off, forged rejections, the precedence of the
    verdicts, and second encodings (a word + its modulus), which are malformed"""
    mine = [c for c in F.cases() if c["key"]["id"] == key_id]
    assert mine
    vkh = forged_vk(mine[0]["key"])
    bad = []
    for c in mine:
        want = F.verdict_in_exponent(c["key"], c)
        assert want == c["want"], c["name"]
        got = vkh.verify(F.verify_input(c))
        if got != want:
            bad.append((c["name"], got, want))
    assert not bad, bad


@pytest.mark.parametrize("shape", [(3, 1), (3, 3)])
def test_batch_of_distinct_forged_proofs(forged_vk, shape):
    """70 proofs with their own public inputs, commitment values and a: entry i must be judged on ITS scalars, pairs and Bs.  Rejections
    of the three kinds at 0, 63, 64, 69; entry 31 is the proof of entry 30 under other public inputs.  Then batches of 1 and 3 in the
    workspace the 70 left behind."""
    B = load_binding()
    key = F.forge_key(*shape)
    vkh = forged_vk(key)
    batch = F.distinct_batch(key, 70, 500 + shape[1])
    want = [F.verdict_in_exponent(key, c) for c in batch]
    assert [want[i] for i in (0, 31, 63, 64, 69)] == [B.VERIFY_MALFORMED, B.VERIFY_PAIRING, B.VERIFY_MALFORMED, B.VERIFY_PEDERSEN, B.VERIFY_MALFORMED]
    assert want.count(B.VERIFY_OK) == 65
    inputs = [F.verify_input(c) for c in batch]
    assert len({x["public_inputs"].tobytes() for x in inputs}) == 70 and len({x["commitment_values"].tobytes() for x in inputs}) == 69
    assert np.array_equal(inputs[30]["raw"], inputs[31]["raw"])
    assert list(vkh.verify_batch(inputs)) == want
    assert [vkh.verify(x) for x in inputs] == want
    for n in (1, 3):
        assert list(vkh.verify_batch(inputs[62:62 + n])) == want[62:62 + n], n
        assert list(vkh.verify_batch(inputs[70 - n:])) == want[70 - n:], n


@pytest.mark.parametrize("entry", ["verify", "verify combined"])
def test_refusal_messages_are_the_same_words_under_each_entry_point(ctx, forged_vk, entry):
    """mi_groth16_verify_batch and mi_groth16_verify_combined over n = 2 proofs of a key with 1 public input and 2 commitments: a null
    vk, input or verdict, n = 2^24 + 1 and each optional pointer left out of proof 1 are refused with MI_EINVAL and the exact message,
    under the entry point's own prefix, and a refusal writes neither a verdict nor first_malformed"""
    key = F.forge_key(2, 2)
    vkh = forged_vk(key)
    lib = ctx.lib
    inp = F.verify_input(F.honest(key, 77))
    assert set(inp) == {"raw", "public_inputs", "commitments", "pok", "commitment_values", "fold_challenge"}
    arr, keep = vkh._inputs([inp, inp])
    out = np.full(2, 255, np.uint8)
    first = C.c_uint64(77)
    vd = out.ctypes.data_as(C.c_void_p)
    if entry == "verify":
        call = lambda vk, a, n, v: lib.mi_groth16_verify_batch(ctx.h, vk, a, C.c_size_t(n), v)
    else:
        call = lambda vk, a, n, v: lib.mi_groth16_verify_combined(ctx.h, vk, a, C.c_size_t(n), bytes(32), v, C.byref(first))

    def refused(message, vk, a, n, v):
        assert call(vk, a, n, v) == -1, message
        assert lib.mi_last_error(ctx.h).decode() == f"{entry}: {message}"
        assert out.tolist() == [255, 255] and first.value == 77, message

    refused("null vk, input or verdict pointer", None, arr, 2, vd)
    refused("null vk, input or verdict pointer", vkh.h, None, 2, vd)
    refused("more than 2^24 proofs in one batch", vkh.h, arr, (1 << 24) + 1, vd)
    refused("null vk, input or verdict pointer", vkh.h, arr, 2, None)
    cv_null = "commitments, pok or commitment_values is null"
    for name, message in (("commitments", cv_null), ("public_inputs", "public_inputs is null"), ("pok", cv_null),
                          ("fold_challenge", "fold_challenge is null with more than one commitment"), ("commitment_values", cv_null)):
        one_out, keep1 = vkh._inputs([inp, {k: x for k, x in inp.items() if k != name}])
        refused(message, vkh.h, one_out, 2, vd)
    assert call(vkh.h, arr, 2, vd) == 0
    assert (out.tolist() == [R.OK, R.OK]) if entry == "verify" else (out[0], first.value) == (R.OK, 2)


def test_vk_load_asks_for_reduced_words_and_takes_infinite_k(ctx):
    B = load_binding()
    key = F.forge_key(3, 1)
    d, nbp, ped = V.vk_arrays(key["vk"])

    def plus_p(arr, row):
        a = np.array(arr, np.uint64, copy=True); rows = a.reshape(-1, 4)
        v = cref.limbs_to_int(rows[row]) + R.p
        assert R.p <= v < 1 << 256
        rows[row] = cref.int_to_limbs(v)
        return a

    # rows of 4 words: alpha1 = x, y; gamma2 = x.a0, x.a1, y.a0, y.a1; k = 2 per point; ped[0] = g (4 rows), g_sigma_neg (4 rows)
    for what, vk, pd in ((r"alpha1 has", dict(d, alpha1=plus_p(d["alpha1"], 0)), ped), (r"gamma2 has", dict(d, gamma2=plus_p(d["gamma2"], 2)), ped),
                         (r"k\[1\] has", dict(d, k=plus_p(d["k"], 3)), ped), (r"ped\[0\]\.g_sigma_neg has", d, plus_p(ped, 5))):
        with pytest.raises(B.MiError, match=what):
            ctx.vk_load(vk, nbp, pd)
    ctx.vk_load(d, nbp, ped).free()
    for shape, zero_k in (((2, 0), (1,)), ((3, 1), (0,))):
        k = F.forge_key(*shape, zero_k=zero_k)
        assert k["vk"]["k"][zero_k[0]] is None
        dd, n, pp = V.vk_arrays(k["vk"])
        ctx.vk_load(dd, n, pp).free()


def test_pedersen_vk_make_at_the_largest_count(ctx):
    key = F.forge_key(2, 16)
    assert np.array_equal(ctx.pedersen_vk_make(fr_arr(key["exps"]["sigma"])), V.vk_arrays(key["vk"])[2])
