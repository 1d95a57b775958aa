"""GPU suite: the sigma half of a phase-2 ceremony (include/mi355x_groth16_phase2_check.h): the state's points [-sigma_k]2,
mi_phase2_contribute_sigma_proved, mi_phase2_verify_adopt_sigma, mi_phase2_get_pedersen_vk, mi_phase2_get_chain_info.

The style is tests/test_gpu_phase2_check.py's.  Every claimed array is built from KNOWN exponents (Python integers, the points by
mi_batch_scalar_mul_g1 / _g2) and every expected mask is computed IN THE EXPONENT with hashlib's coefficients: commitment k's relation
reads sum_i r_i (t_ki g'_k + b'_ki) = 0 mod r for the basis exponents t_ki, the claimed BasisExpSigma exponents b'_ki and the claimed
[g'_k]2.  The steps of the chain are restated by tests/phase2_sigma_ref.py (hashlib, oracle/pyref.py's group law over the twist).  The
yardstick shares nothing with the device's MSM and pairing.  Every comparison is exact.

Commitment sizes: 1 (an MSM of one term), 64 and 65 (one lane past a 64-lane block of the scale kernel and of the coefficient
kernel), one and two commitments.

1  a proved step equals the plain one, and its bytes the restatement's
2  a two-party ceremony: delta and sigma steps interleaved, adopted all at once and step by step; the streams equal Setup's
3  tampers, each against the model's mask; the state is as it was
4  refusals leave the state alone
5  the sealed key of an adopted state proves, verifies and passes the audit
6  host buffers between guard bands; a call's result after a larger call"""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import setup_cases as SC
import r1cs_cases as RC
import bytes_cases as BC
import verify_cases as V
import banded as BD
import phase2_sigma_ref as S
import test_gpu_phase2 as T2
import test_gpu_phase2_check as TG
import test_phase2_check_cpu as TC
from helpers import fr_arr, fr_vals, g1_arr, g1_pts, g2_arr
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R = P.R_MOD
SEED_A, SEED_B = TG.SEED_A, TG.SEED_B
ID0, ID1 = TC.ID0, TC.ID1
NC, NB_PUBLIC = 100, 5    # the circuit of tests/test_gpu_phase2_check.py: N = 128
S1, S2, S3 = (T2.secrets(1800 + i, 2)[3] for i in range(3))      # the factors of three steps, one per commitment
N1, N2, N3 = (T2.secrets(1810 + i, 2)[3] for i in range(3))      # their nonces
D1, K1 = TG.D1, TG.K1
R_WORDS = np.frombuffer(R.to_bytes(32, "little"), np.uint64)


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def circuit(ncom, n_committed):
    return SC.synth_r1cs(NC, nb_wires=160, nb_public=NB_PUBLIC, seed=1603, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=ncom,
                         n_committed=n_committed)


_inputs = {}


def inputs(ctx, ncom, n_committed, unit_sigma=False):
    """(r1cs, srs, trapdoor values, sigma0 as integers, sigma0 as the library's rows), made once per shape"""
    key = (ncom, n_committed, unit_sigma)
    if key not in _inputs:
        tau, alpha, beta, sigma0 = T2.secrets(1600, ncom)
        if unit_sigma:
            sigma0 = [1] * ncom
        _inputs[key] = (circuit(ncom, n_committed), T2.make_srs(ctx, NC, tau, alpha, beta), (tau, alpha, beta), sigma0, [fr_arr([x])[0] for x in sigma0])
    return _inputs[key]


def all_arrays(ctx, B, st, ncom):
    names = [B.PHASE2_G1_A, B.PHASE2_G1_B, B.PHASE2_G2_B, B.PHASE2_G1_K, B.PHASE2_G1_Z, B.PHASE2_VK_K] + [B.PHASE2_BASIS + j for j in range(2 * ncom)]
    return [ctx.phase2_array(st, w) for w in names]


def sigma_claim_of(ctx, B, st, ncom):
    """what a contributor to sigma hands over: the state's BasisExpSigma arrays and its points [-sigma_k]2"""
    return {"bes": [ctx.phase2_array(st, B.PHASE2_BASIS + 2 * k + 1) for k in range(ncom)], "gs": ctx.phase2_get_pedersen_vk(st, ncom)[:, 1].copy()}


def adopt_sigma(ctx, st, claim, steps, hashes, seed=SEED_A):
    return ctx.phase2_verify_adopt_sigma(st, claim["bes"], claim["gs"], np.stack(steps), hashes, seed)


def snapshot(ctx, st):
    """the state as a caller can see it: the RAW streams, both chain values and both counts"""
    return ctx.phase2_to_streams(st, T2.RAW), ctx.phase2_chain_info(st)


def neg_points(exps):
    return [P.g2_mul(P.G2_GEN, (R - e) % R) for e in exps]


# ---------------------------------------------------------------------------------------------------- 1: a proved step equals the plain one
@pytest.mark.parametrize("ncom,n_committed", [(1, 1), (2, 64), (2, 65)])
def test_proved_sigma_step_equals_the_plain_one(ctx, ncom, n_committed):
    B = load_binding()
    r1cs, srs, (tau, alpha, beta), sigma0, sg = inputs(ctx, ncom, n_committed)
    s, n = S1[:ncom], N1[:ncom]
    st, twin = ctx.phase2_init(r1cs, srs, sg), ctx.phase2_init(r1cs, srs, sg)
    try:
        info = ctx.phase2_chain_info(st)
        assert info == {"n_commitments": ncom, "n_records": 0, "chain": ID0, "n_sigma_records": 0, "sigma_chain": ID0}
        vk0 = ctx.phase2_get_pedersen_vk(st, ncom)
        assert np.array_equal(vk0, ctx.pedersen_vk_make(fr_arr(sigma0))), "mi_phase2_init makes the points as mi_pedersen_vk_make does"
        step, h = ctx.phase2_contribute_sigma_proved(st, fr_arr(s), fr_arr(n))
        ctx.phase2_contribute(twin, fr_arr([1])[0], fr_arr(s))
        for got, want in zip(all_arrays(ctx, B, st, ncom), all_arrays(ctx, B, twin, ncom)):
            assert np.array_equal(got, want)
        sigma = [a * b % R for a, b in zip(sigma0, s)]
        want_vk = ctx.pedersen_vk_make(fr_arr(sigma))
        assert np.array_equal(ctx.phase2_get_pedersen_vk(st, ncom), want_vk) and np.array_equal(ctx.phase2_get_pedersen_vk(twin, ncom), want_vk)
        assert ctx.phase2_to_streams(st, T2.RAW) == ctx.phase2_to_streams(twin, T2.RAW)
        # with given nonces the step is the restatement's, byte for byte
        steps, e_end = S.chain(ID0, 0, [(R - x) % R for x in sigma0], [list(zip(s, n))])
        pr, hs = S.proofs_array(steps)
        assert np.array_equal(step, pr[0]) and h == hs[0] and e_end == [(R - x) % R for x in sigma]
        assert np.array_equal(step[:, :16], want_vk[:, 1])
        assert B.phase2_sigma_records_verify(vk0[:, 1], ID0, 0, step[None], [h]) == 1
        # nothing that depends on delta has moved: Z, K, delta1, delta2 are Setup's for delta = 1, and the delta chain stands at its start
        T2.assert_equals_setup(ctx, r1cs, st, T2.trapdoor(tau, alpha, beta, 1, sigma), encodings=(T2.RAW,))
        info = ctx.phase2_chain_info(st)
        assert info == {"n_commitments": ncom, "n_records": 0, "chain": ID0, "n_sigma_records": 1, "sigma_chain": h}
        assert ctx.phase2_chain_info(twin)["n_sigma_records"] == 0, "the plain contribution leaves no record"
        rec = ctx.phase2_contribute_proved(st, fr_arr([D1])[0], fr_arr([K1])[0])
        assert np.array_equal(rec, TC.records_array(TC.chain(ID0, 0, 1, [(D1, K1)]))[0])
        info = ctx.phase2_chain_info(st)
        assert (info["n_records"], info["chain"], info["n_sigma_records"], info["sigma_chain"]) == (1, rec[20:].tobytes(), 1, h)
    finally:
        ctx.phase2_free(st); ctx.phase2_free(twin)


# ---------------------------------------------------------------------------------------------------- 2: a two-party ceremony
@pytest.mark.parametrize("ncom,n_committed", [(1, 1), (1, 64), (2, 65)])
def test_two_party_ceremony_ends_in_setups_key(ctx, ncom, n_committed):
    """init with sigma = 1, then a delta step, a sigma step and a second sigma step on the contributor; the verifier's own state adopts
    them and is never handed a sigma scalar"""
    B = load_binding()
    r1cs, srs, (tau, alpha, beta), sigma0, sg = inputs(ctx, ncom, n_committed, unit_sigma=True)
    s1, s2, s3, n1, n2, n3 = (x[:ncom] for x in (S1, S2, S3, N1, N2, N3))
    states = [ctx.phase2_init(r1cs, srs, sg) for _ in range(3)]
    c, v_all, v_step = states
    try:
        rec = ctx.phase2_contribute_proved(c, fr_arr([D1])[0], fr_arr([K1])[0])
        claim_d = TG.claim_of(ctx, B, c, D1)
        step1, h1 = ctx.phase2_contribute_sigma_proved(c, fr_arr(s1), fr_arr(n1))
        claim1 = sigma_claim_of(ctx, B, c, ncom)
        step2, h2 = ctx.phase2_contribute_sigma_proved(c, fr_arr(s2), fr_arr(n2))
        claim2 = sigma_claim_of(ctx, B, c, ncom)
        steps, _ = S.chain(ID0, 0, [R - 1] * ncom, [list(zip(s1, n1)), list(zip(s2, n2))])
        pr, hs = S.proofs_array(steps)
        assert np.array_equal(np.stack([step1, step2]), pr) and [h1, h2] == hs
        sigma = [a * b % R for a, b in zip(s1, s2)]
        td = T2.trapdoor(tau, alpha, beta, D1, sigma)
        T2.assert_equals_setup(ctx, r1cs, c, td, encodings=(T2.COMPRESSED,))
        # all at once
        assert TG.adopt(ctx, v_all, claim_d, [rec]) == (0, 1)
        assert adopt_sigma(ctx, v_all, claim2, [step1, step2], [h1, h2]) == (0, 0, 2)
        print(f"verify_adopt_sigma {ncom} x {n_committed}: {ctx.srs_check_stats(verify=True)}")
        T2.assert_equals_setup(ctx, r1cs, v_all, td)    # both encodings, byte for byte
        assert np.array_equal(ctx.phase2_get_pedersen_vk(v_all, ncom), ctx.pedersen_vk_make(fr_arr(sigma)))
        # step by step, sigma before delta; the later sigma step does not verify before the earlier one is adopted
        before = snapshot(ctx, v_step)
        assert adopt_sigma(ctx, v_step, claim2, [step2], [h2]) == (B.PHASE2_BAD_SIGMA_RECORD, 0, 0)
        assert snapshot(ctx, v_step) == before
        assert adopt_sigma(ctx, v_step, claim1, [step1], [h1]) == (0, 0, 1)
        T2.assert_equals_setup(ctx, r1cs, v_step, T2.trapdoor(tau, alpha, beta, 1, s1), encodings=(T2.COMPRESSED,))
        assert TG.adopt(ctx, v_step, claim_d, [rec]) == (0, 1)
        assert adopt_sigma(ctx, v_step, claim2, [step2], [h2], seed=None) == (0, 0, 1)     # the operating system's seed
        for enc in (T2.RAW, T2.COMPRESSED):
            assert ctx.phase2_to_streams(v_step, enc) == ctx.phase2_to_streams(v_all, enc)
        info = ctx.phase2_chain_info(v_step)
        assert (info["n_records"], info["chain"], info["n_sigma_records"], info["sigma_chain"]) == (1, rec[20:].tobytes(), 2, h2)
        # the adopted chain goes on: a third step made on the adopter verifies for the contributor
        step3, h3 = ctx.phase2_contribute_sigma_proved(v_step, fr_arr(s3), fr_arr(n3))
        want3, _ = S.chain(h2, 2, [(R - x) % R for x in sigma], [list(zip(s3, n3))])
        pr3, hs3 = S.proofs_array(want3)
        assert np.array_equal(step3, pr3[0]) and h3 == hs3[0]
        assert adopt_sigma(ctx, c, sigma_claim_of(ctx, B, v_step, ncom), [step3], [h3]) == (0, 0, 1)
        assert ctx.phase2_to_streams(c, T2.RAW) == ctx.phase2_to_streams(v_step, T2.RAW)
        T2.assert_equals_setup(ctx, r1cs, c, T2.trapdoor(tau, alpha, beta, D1, [a * b % R for a, b in zip(sigma, s3)]), encodings=(T2.RAW,))
        # a nonce from the operating system: the step holds all the same
        step4, h4 = ctx.phase2_contribute_sigma_proved(c, fr_arr([5] * ncom))
        assert B.phase2_sigma_records_verify(step3[:, :16], h3, 3, step4[None], [h4]) == 1
        assert S.first_bad([p[0] for p in S.parts_of(step3)], h3, 3, [step4], [h4]) == 1
    finally:
        for s in states:
            ctx.phase2_free(s)


# ---------------------------------------------------------------------------------------------------- 3: tampers, every exponent known
@pytest.fixture(scope="module")
def ceremony(ctx):
    """two commitments of 65 wires: a contributor's state after two proved sigma steps, the basis in the exponent, a verifier's fresh state"""
    ncom, n_committed = 2, 65
    r1cs, srs, (tau, alpha, beta), sigma0, sg = inputs(ctx, ncom, n_committed)
    st, v = ctx.phase2_init(r1cs, srs, sg), ctx.phase2_init(r1cs, srs, sg)
    made = [ctx.phase2_contribute_sigma_proved(st, fr_arr(S1), fr_arr(N1)), ctx.phase2_contribute_sigma_proved(st, fr_arr(S2), fr_arr(N2))]
    _, t = TG.circuit_exponents(r1cs, tau, alpha, beta)
    basis = [[t[int(w) - NB_PUBLIC] for w in ws] for ws, _ in r1cs["commitments"]]
    sigma = [a * b % R * c % R for a, b, c in zip(sigma0, S1, S2)]
    yield {"ncom": ncom, "n": n_committed, "r1cs": r1cs, "srs": srs, "sg": sg, "sigma0": sigma0, "sigma": sigma, "st": st, "v": v, "basis": basis,
           "steps": [m[0] for m in made], "hashes": [m[1] for m in made], "trapdoor": (tau, alpha, beta)}
    ctx.phase2_free(st); ctx.phase2_free(v)


def claim_from_exponents(ctx, bes, gs):
    return {"bes": [ctx.batch_scalar_mul(D.G1, fr_arr(b)) for b in bes], "gs": ctx.batch_scalar_mul(D.G2, fr_arr(gs), g2=True)}


def honest_exponents(cer):
    return [[x * sg % R for x in b] for b, sg in zip(cer["basis"], cer["sigma"])], [(R - sg) % R for sg in cer["sigma"]]


def adopt_model(B, cer, bes, gs, steps, hashes, seed, start_hash=ID0):
    """mi_phase2_verify_adopt_sigma for the verifier's fresh state (sigma0, no step yet) in the exponent -> (mask, bad_commitments, first_bad)"""
    mask, bad = 0, 0
    fb = S.first_bad(neg_points(cer["sigma0"]), start_hash, 0, steps, hashes)
    if fb != len(hashes):
        mask |= B.PHASE2_BAD_SIGMA_RECORD
    last = S.parts_of(steps[-1])
    for k, g in enumerate(gs):
        if P.g2_mul(P.G2_GEN, g) != last[k][0]:
            mask |= B.PHASE2_BAD_SIGMA_LINK
        if sum(TC.coeff(seed, i) * (t * g + b) for i, (t, b) in enumerate(zip(cer["basis"][k], bes[k]))) % R:
            mask |= B.PHASE2_BAD_BES
            bad |= 1 << k
    return mask, bad, fb


def test_the_sigma_exponents_are_the_states(ctx, ceremony):
    """the model's basis is the verifier's Basis arrays, and times sigma the contributor's BasisExpSigma; its points are the state's"""
    B = load_binding()
    cer = ceremony
    for k in range(cer["ncom"]):
        assert np.array_equal(ctx.batch_scalar_mul(D.G1, fr_arr(cer["basis"][k])), ctx.phase2_array(cer["v"], B.PHASE2_BASIS + 2 * k))
        assert any(cer["basis"][k]) and len(cer["basis"][k]) == cer["n"]
    honest = claim_from_exponents(ctx, *honest_exponents(cer))
    mine = sigma_claim_of(ctx, B, cer["st"], cer["ncom"])
    assert all(np.array_equal(a, b) for a, b in zip(honest["bes"], mine["bes"])) and np.array_equal(honest["gs"], mine["gs"])
    for seed in (SEED_A, SEED_B):
        assert adopt_model(B, cer, *honest_exponents(cer), cer["steps"], cer["hashes"], seed) == (0, 0, 2)


def _bump(bes, k, i, by=1):
    out = [list(b) for b in bes]
    out[k][i] = (out[k][i] + by) % R
    return out


def _tampers(B, cer):
    """name -> (claimed BasisExpSigma exponents, claimed g_sigma_neg exponents, the steps, the hashes, the stated (mask, bad_commitments, first_bad))"""
    bes, gs = honest_exponents(cer)
    steps, hashes = cer["steps"], cer["hashes"]
    BES, LINK, REC = B.PHASE2_BAD_BES, B.PHASE2_BAD_SIGMA_LINK, B.PHASE2_BAD_SIGMA_RECORD
    at_inf = [list(b) for b in bes]; at_inf[0][5] = 0
    other = [(gs[0] + R - 1) % R, gs[1]]                      # [-(sigma_0 + 1)]2
    wrong = steps[1].copy(); wrong[1, 32:] = fr_arr([(fr_vals(steps[1][1, 32:])[0] + 1) % R])[0]
    other_id, _ = S.chain(ID1, 0, [(R - x) % R for x in cer["sigma0"]], [list(zip(S1, N1)), list(zip(S2, N2))])
    pr_id, hs_id = S.proofs_array(other_id)
    return {
        "BES[0][0]": (_bump(bes, 0, 0), gs, steps, hashes, (BES, 1, 2)),
        "BES[1][63]": (_bump(bes, 1, 63), gs, steps, hashes, (BES, 2, 2)),
        "BES[1][64]": (_bump(bes, 1, 64), gs, steps, hashes, (BES, 2, 2)),
        "BES[0][last]": (_bump(bes, 0, cer["n"] - 1), gs, steps, hashes, (BES, 1, 2)),
        "BES[0][5] at infinity": (at_inf, gs, steps, hashes, (BES, 1, 2)),
        "a defect in each commitment": (_bump(_bump(bes, 0, 7), 1, 9), gs, steps, hashes, (BES, 3, 2)),
        "g_sigma_neg of another sigma": (bes, other, steps, hashes, (LINK | BES, 1, 2)),
        "both scaled by a factor no step covers": ([[x * 3 % R for x in b] for b in bes], [g * 3 % R for g in gs], steps, hashes, (LINK, 0, 2)),
        "a wrong response": (bes, gs, [steps[0], wrong], hashes, (REC, 0, 1)),
        "one byte of the first hash": (bes, gs, steps, [bytes([hashes[0][0] ^ 1]) + hashes[0][1:], hashes[1]], (REC, 0, 0)),
        "steps of another transcript id": (bes, gs, list(pr_id), hs_id, (REC, 0, 0)),
    }


TAMPER_NAMES = ("BES[0][0]", "BES[1][63]", "BES[1][64]", "BES[0][last]", "BES[0][5] at infinity", "a defect in each commitment", "g_sigma_neg of another sigma",
                "both scaled by a factor no step covers", "a wrong response", "one byte of the first hash", "steps of another transcript id")


@pytest.mark.parametrize("name", TAMPER_NAMES)
def test_a_tampered_sigma_claim_gives_its_bits(ctx, ceremony, name):
    B = load_binding()
    cer = ceremony
    bes, gs, steps, hashes, stated = _tampers(B, cer)[name]
    claim = claim_from_exponents(ctx, bes, gs)
    before = snapshot(ctx, cer["v"])
    for seed in (SEED_A, SEED_B):
        assert adopt_model(B, cer, bes, gs, steps, hashes, seed) == stated, "the model in the exponent against the stated mask"
        assert adopt_sigma(ctx, cer["v"], claim, steps, hashes, seed) == stated
        assert snapshot(ctx, cer["v"]) == before


def test_two_defects_that_cancel_under_one_seed(ctx, ceremony):
    """r_3 d_3 + r_64 d_64 = 0 for SEED_A's coefficients and not for SEED_B's: the model decides each mask.  Under the seed its maker
    could predict the claim passes and IS adopted -- the header's warning about a fixed seed -- so the verifier here is a state of its own."""
    B = load_binding()
    cer = ceremony
    bes, gs = honest_exponents(cer)
    d64 = (R - TC.coeff(SEED_A, 3)) * P.fr_inv(TC.coeff(SEED_A, 64)) % R
    bes = _bump(_bump(bes, 1, 3), 1, 64, d64)
    claim = claim_from_exponents(ctx, bes, gs)
    w = ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"])
    try:
        before = snapshot(ctx, w)
        want_b = adopt_model(B, cer, bes, gs, cer["steps"], cer["hashes"], SEED_B)
        assert want_b == (B.PHASE2_BAD_BES, 2, 2)
        assert adopt_sigma(ctx, w, claim, cer["steps"], cer["hashes"], SEED_B) == want_b and snapshot(ctx, w) == before
        want_a = adopt_model(B, cer, bes, gs, cer["steps"], cer["hashes"], SEED_A)
        assert want_a == (0, 0, 2)
        assert adopt_sigma(ctx, w, claim, cer["steps"], cer["hashes"], SEED_A) == want_a
    finally:
        ctx.phase2_free(w)


def test_a_sigma_advanced_without_a_record_does_not_verify(ctx, ceremony):
    """plain mi_phase2_contribute moves [-sigma]2 and leaves the sigma chain where it was: the next step starts from points nobody else has"""
    B = load_binding()
    cer = ceremony
    p = ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"])
    try:
        ctx.phase2_contribute(p, fr_arr([1])[0], fr_arr(S1))
        step, h = ctx.phase2_contribute_sigma_proved(p, fr_arr(S2), fr_arr(N2))
        want, _ = S.chain(ID0, 0, [(R - a * b) % R for a, b in zip(cer["sigma0"], S1)], [list(zip(S2, N2))])   # index 0, from [-sigma0 s1]2
        assert np.array_equal(step, S.proofs_array(want)[0][0]) and h == want[0][1]
        model = adopt_model(B, cer, *honest_exponents(cer), [step], [h], SEED_A)
        assert model == (B.PHASE2_BAD_SIGMA_RECORD, 0, 0)
        before = snapshot(ctx, cer["v"])
        assert adopt_sigma(ctx, cer["v"], sigma_claim_of(ctx, B, p, cer["ncom"]), [step], [h]) == model
        assert snapshot(ctx, cer["v"]) == before
    finally:
        ctx.phase2_free(p)


def test_transcript_id_starts_both_chains(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    a, b = (ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"]) for _ in range(2))
    try:
        ctx.phase2_set_transcript_id(a, ID1)
        made = [ctx.phase2_contribute_sigma_proved(a, fr_arr(S1), fr_arr(N1)), ctx.phase2_contribute_sigma_proved(a, fr_arr(S2), fr_arr(N2))]
        want, _ = S.chain(ID1, 0, [(R - x) % R for x in cer["sigma0"]], [list(zip(S1, N1)), list(zip(S2, N2))])
        pr, hs = S.proofs_array(want)
        assert np.array_equal(np.stack([m[0] for m in made]), pr) and [m[1] for m in made] == hs
        with pytest.raises(B.MiError, match="transcript id"):     # a sigma step counts as a record of the state
            ctx.phase2_set_transcript_id(a, ID0)
        rec = ctx.phase2_contribute_proved(a, fr_arr([D1])[0], fr_arr([K1])[0])    # the delta chain starts from the same id
        assert np.array_equal(rec, TC.records_array(TC.chain(ID1, 0, 1, [(D1, K1)]))[0])
        claim = sigma_claim_of(ctx, B, a, cer["ncom"])
        assert adopt_sigma(ctx, b, claim, list(pr), hs) == (B.PHASE2_BAD_SIGMA_RECORD, 0, 0)    # b's chains start from the zero id
        ctx.phase2_set_transcript_id(b, ID1)
        assert adopt_sigma(ctx, b, claim, list(pr), hs) == (0, 0, 2)
        with pytest.raises(B.MiError, match="transcript id"):     # an adopted step counts
            ctx.phase2_set_transcript_id(b, ID1)
    finally:
        ctx.phase2_free(a); ctx.phase2_free(b)


# ---------------------------------------------------------------------------------------------------- 4: refusals
def test_sigma_refusals_leave_the_state_alone(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    ncom, steps, hashes = cer["ncom"], cer["steps"], cer["hashes"]
    v = ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"])     # a verifier of its own: this test ends by adopting
    p = ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"])
    bare = ctx.phase2_init(circuit(0, 0), cer["srs"])           # a state without commitments
    lib = ctx.lib
    try:
        good = sigma_claim_of(ctx, B, cer["st"], ncom)
        before = snapshot(ctx, v)
        ledger = ctx.mem_ledger()

        def refused(claim, *words):
            with pytest.raises(B.MiError) as ei:
                adopt_sigma(ctx, v, claim, steps, hashes)
            assert "rc=-1:" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
            assert snapshot(ctx, v) == before and ctx.mem_ledger() == ledger
        refused(dict(good, bes=[good["bes"][0], good["bes"][1][:-1]]), "claim.n[1]", "64", "65")
        off = [b.copy() for b in good["bes"]]; off[1][64, 4] ^= np.uint64(1); off[1][30, 4] ^= np.uint64(1)
        refused(dict(good, bes=off), "claim.basis_exp_sigma[1][30]")
        off = [b.copy() for b in good["bes"]]; off[0][64, 0] ^= np.uint64(2)
        refused(dict(good, bes=off), "claim.basis_exp_sigma[0][64]")
        gs = good["gs"].copy(); gs[1] = g2_arr([V.twist_point_outside_subgroup()])[0]
        refused(dict(good, gs=gs), "claim.g_sigma_neg[1]", "r-torsion")
        gs = good["gs"].copy(); gs[0, 8] ^= np.uint64(1)
        refused(dict(good, gs=gs), "claim.g_sigma_neg[0]", "not on its curve")
        gs = good["gs"].copy(); gs[1] = 0
        refused(dict(good, gs=gs), "claim.g_sigma_neg[1]", "infinity")
        with pytest.raises(B.MiError, match="m is 0"):
            ctx.phase2_verify_adopt_sigma(v, good["bes"], good["gs"], np.zeros((0, ncom, S.WORDS), np.uint64), [], SEED_A)
        with pytest.raises(B.MiError, match="no commitments"):
            ctx.phase2_verify_adopt_sigma(bare, [], np.zeros((1, 16), np.uint64), np.zeros((1, 1, S.WORDS), np.uint64), [bytes(32)], SEED_A)
        # null arguments, through the C-ABI directly: nothing is written
        pr = np.stack(steps); hbuf = (C.c_uint8 * 64).from_buffer_copy(b"".join(hashes))
        failed, bad, fb = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
        ptrs = (C.c_void_p * ncom)(*[a.ctypes.data for a in good["bes"]]); counts = (C.c_uint64 * ncom)(*[a.shape[0] for a in good["bes"]])
        cl = B.Phase2SigmaClaim(C.cast(ptrs, C.c_void_p), C.cast(counts, C.c_void_p), good["gs"].ctypes.data)
        args = [ctx.h, v, C.byref(cl), B._p(pr), hbuf, C.c_size_t(2), SEED_A, C.byref(failed), C.byref(bad), C.byref(fb)]
        for hole in (0, 1, 2, 3, 4, 7, 8):
            a = list(args); a[hole] = None
            assert lib.mi_phase2_verify_adopt_sigma(*a) == -1
        for field in ("basis_exp_sigma", "n", "g_sigma_neg"):
            broken = B.Phase2SigmaClaim(cl.basis_exp_sigma, cl.n, cl.g_sigma_neg); setattr(broken, field, None)
            a = list(args); a[2] = C.byref(broken)
            assert lib.mi_phase2_verify_adopt_sigma(*a) == -1
        assert (failed.value, bad.value, fb.value) == (7, 7, 7) and snapshot(ctx, v) == before and ctx.mem_ledger() == ledger
        # mi_phase2_contribute_sigma_proved: a factor or a nonce that is 0 or not below r, a null argument, a state without commitments
        p_before = snapshot(ctx, p)
        at_r = fr_arr(S1); at_r[1] = R_WORDS
        for sf, nn, word in ((fr_arr([S1[0], 0]), fr_arr(N1), "sigma_factor[1] is 0"), (at_r, fr_arr(N1), "sigma_factor[1] is not below r"),
                             (fr_arr(S1), fr_arr([0, N1[1]]), "nonce is 0"), (fr_arr(S1), np.stack([fr_arr(N1)[0], R_WORDS]), "nonce is not below r")):
            with pytest.raises(B.MiError, match=word.replace("[", r"\[").replace("]", r"\]")):
                ctx.phase2_contribute_sigma_proved(p, sf, nn)
        out = np.zeros((ncom, S.WORDS), np.uint64); h = (C.c_uint8 * 32)()
        sfp, nnp = fr_arr(S1), fr_arr(N1)
        assert lib.mi_phase2_contribute_sigma_proved(ctx.h, p, None, B._p(nnp), B._p(out), h) == -1
        assert lib.mi_phase2_contribute_sigma_proved(ctx.h, p, B._p(sfp), B._p(nnp), None, h) == -1
        assert lib.mi_phase2_contribute_sigma_proved(ctx.h, p, B._p(sfp), B._p(nnp), B._p(out), None) == -1
        assert lib.mi_phase2_contribute_sigma_proved(ctx.h, None, B._p(sfp), B._p(nnp), B._p(out), h) == -1
        assert lib.mi_phase2_contribute_sigma_proved(ctx.h, bare, B._p(sfp), B._p(nnp), B._p(out), h) == -1 and b"no commitments" in lib.mi_last_error(ctx.h)
        assert not out.any() and bytes(h) == bytes(32) and snapshot(ctx, p) == p_before
        assert lib.mi_phase2_get_pedersen_vk(ctx.h, None, B._p(out)) == -1 and lib.mi_phase2_get_pedersen_vk(ctx.h, p, None) == -1
        assert lib.mi_phase2_get_pedersen_vk(ctx.h, bare, None) == 0 and lib.mi_phase2_get_chain_info(ctx.h, p, None) == -1
        # the chain did not move either: the state's first step is step 0 of the zero id
        step, h0 = ctx.phase2_contribute_sigma_proved(p, fr_arr(S1), fr_arr(N1))
        assert np.array_equal(step, steps[0]) and h0 == hashes[0]
        # and the verifier's state, untouched through all of it, still adopts the honest claim
        assert snapshot(ctx, v) == before
        assert adopt_sigma(ctx, v, good, steps, hashes) == (0, 0, 2)
        assert ctx.phase2_to_streams(v, T2.RAW) == ctx.phase2_to_streams(cer["st"], T2.RAW)
    finally:
        for s in (v, p, bare):
            ctx.phase2_free(s)


# ---------------------------------------------------------------------------------------------------- 5: the key works
def test_adopted_sigma_key_proves_verifies_and_passes_the_audit(ctx):
    """tests/test_gpu_phase2.py's test_phase2_sealed_key_proves_and_verifies with a ceremony in front: sigma starts at 1, a delta step and a
    sigma step are adopted by a verifier, and the verifier's sealed key with mi_phase2_get_pedersen_vk's pairs is loaded by mi_vk_load"""
    B = load_binding()
    ncom, n, nab, nb_public = 1, 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 41, long_lens=(16, 17, 64), commitments=ncom, n_committed=7)
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 42)
    tau, alpha, beta, _ = T2.secrets(1700, ncom)
    delta, k = T2.secrets(1701, 1)[:2]
    rr, ss = cref.gen_scalars(2, 61, 0)
    srs = T2.make_srs(ctx, n, tau, alpha, beta)
    one = [fr_arr([1])[0]]
    c, v = ctx.phase2_init(r1cs, srs, one), ctx.phase2_init(r1cs, srs, one)
    pool = B.Prover(0, 1)
    keys, vkh, claim = [], None, None
    try:
        rec = ctx.phase2_contribute_proved(c, fr_arr([delta])[0], fr_arr([k])[0])
        assert TG.adopt(ctx, v, TG.claim_of(ctx, B, c, delta), [rec]) == (0, 1)
        step, h = ctx.phase2_contribute_sigma_proved(c, fr_arr(S1[:1]))
        assert adopt_sigma(ctx, v, sigma_claim_of(ctx, B, c, ncom), [step], [h], seed=None) == (0, 0, 1)
        keys.append(ctx.phase2_seal(v, nb_public + ncom, ncom))
        keys.append(ctx.setup(r1cs, T2.trapdoor(tau, alpha, beta, delta, S1[:1])))
        (pkh, peds, vk), (ref, ref_peds, _) = keys
        ped_vk = ctx.phase2_get_pedersen_vk(v, ncom)
        assert np.array_equal(ped_vk, ctx.pedersen_vk_make(fr_arr(S1[:1])))
        vkh = ctx.vk_load(vk, nb_public, ped_vk)
        pub = fr_vals(W[1:nb_public])
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
        cms = np.stack([pool.commit(peds[j], vals[j]).reshape(8) for j in range(ncom)])
        assert np.array_equal(cms, np.stack([pool.commit(ref_peds[j], vals[j]).reshape(8) for j in range(ncom)]))
        values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
        for (_, cw), val in zip(r1cs["commitments"], values):
            W[cw] = fr_arr([val])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        proofs = []
        for key, key_peds in ((pkh, peds), (ref, ref_peds)):
            proof, _ = pool.wait(pool.submit_bsb22(key, W, a, b, None, rr, ss, [(key_peds[j], vals[j]) for j in range(ncom)], fr_arr([fold])[0]))
            proofs.append(proof)
        assert np.array_equal(proofs[0]["raw"], proofs[1]["raw"]) and np.array_equal(proofs[0]["pok"], proofs[1]["pok"])
        item = {"raw": proofs[0]["raw"], "public_inputs": np.ascontiguousarray(W[1:nb_public]), "commitments": cms,
                "pok": np.ascontiguousarray(proofs[0]["pok"]).reshape(8), "commitment_values": fr_arr(values)}
        assert vkh.verify(item) == B.VERIFY_OK == 0
        assert vkh.verify(dict(item, pok=g1_arr([P.g1_mul(P.G1_GEN, 5)])[0])) == B.VERIFY_PEDERSEN == 2
        claim = ctx.key_claim_from_phase2(v)
        assert ctx.key_audit(r1cs, claim, srs=srs, seed=SEED_A) == 0
    finally:
        if claim is not None:
            ctx.key_claim_free(claim)
        if vkh is not None:
            vkh.free()
        pool.close()
        for pkh, peds, _ in keys:
            T2.free_key(ctx, pkh, peds)
        ctx.phase2_free(c); ctx.phase2_free(v)


# ---------------------------------------------------------------------------------------------------- 6: bounds and history
class HostBand:
    """tests/banded.py's layout and byte stream over HOST memory, for calls whose pointers are host pointers: guard | 32 bytes | payload | guard
    from a 64-byte aligned base, so the payload starts on a 32-byte boundary that is no 64-byte boundary"""

    def __init__(self, payload, name, seed):
        payload = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
        self.name, self.nbytes, self.seed = name, payload.nbytes, seed
        self.off, self.total = BD.layout(self.nbytes)
        raw = np.zeros(self.total + 64, np.uint8)
        shift = (-raw.ctypes.data) % 64
        self.buf = raw[shift:shift + self.total]
        self.buf[:] = BD.pattern(self.total, seed)
        self.buf[self.off:self.off + self.nbytes] = payload
        self.want = payload.copy()
        self.ptr = self.buf.ctypes.data + self.off
        assert self.ptr % 64 == 32

    def arg(self):
        return C.c_void_p(self.ptr)

    def payload(self, dtype=np.uint64):
        return self.buf[self.off:self.off + self.nbytes].copy().view(dtype)

    def check(self):
        want = BD.pattern(self.total, self.seed)
        end = self.off + self.nbytes
        msgs = [BD.describe(self.buf[:self.off], want[:self.off], "before"), BD.describe(self.buf[end:], want[end:], "after")]
        assert not [m for m in msgs if m], f"{self.name}: {msgs}"

    def assert_unchanged(self):
        self.check()
        assert np.array_equal(self.buf[self.off:self.off + self.nbytes], self.want), f"{self.name}: a const input was written"


def test_sigma_calls_between_guard_bands(ctx, ceremony):
    """the claim's arrays, the proofs and the outputs of the three calls that take a context sit between guard bands at 32-byte alignment:
    only outputs are written, and no byte beside them"""
    B = load_binding()
    cer = ceremony
    ncom, lib = cer["ncom"], ctx.lib
    p, w = (ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"]) for _ in range(2))
    seeds = iter(range(0x7361, 0x7400))
    band = lambda arr, name: HostBand(arr, name, next(seeds))
    try:
        # mi_phase2_contribute_sigma_proved, twice
        made = []
        for s, n in ((S1, N1), (S2, N2)):
            sf, nn = band(fr_arr(s), "sigma_factor"), band(fr_arr(n), "nonce")
            out, h = band(np.zeros(ncom * S.WORDS, np.uint64), "out"), band(np.zeros(32, np.uint8), "hash_out")
            assert lib.mi_phase2_contribute_sigma_proved(ctx.h, p, sf.arg(), nn.arg(), out.arg(), h.arg()) == 0
            sf.assert_unchanged(); nn.assert_unchanged(); out.check(); h.check()
            made.append((out.payload().reshape(ncom, S.WORDS), h.payload(np.uint8).tobytes()))
        assert all(np.array_equal(m[0], st) and m[1] == hh for m, st, hh in zip(made, cer["steps"], cer["hashes"]))
        # mi_phase2_get_pedersen_vk
        pv = band(np.zeros(ncom * 32, np.uint64), "pedersen vk out")
        assert lib.mi_phase2_get_pedersen_vk(ctx.h, p, pv.arg()) == 0
        pv.check()
        assert np.array_equal(pv.payload().reshape(ncom, 2, 16), ctx.pedersen_vk_make(fr_arr(cer["sigma"])))
        # mi_phase2_verify_adopt_sigma: a tampered claim (a verdict, nothing adopted), then the honest one
        good = sigma_claim_of(ctx, B, p, ncom)
        bad_bes = [b.copy() for b in good["bes"]]; bad_bes[1][64] = good["bes"][1][0]
        for bes, want in ((bad_bes, (B.PHASE2_BAD_BES, 2, 2)), (good["bes"], (0, 0, 2))):
            arrays = [band(b, f"basis_exp_sigma[{k}]") for k, b in enumerate(bes)]
            ptrs = band(np.array([a.ptr for a in arrays], np.uint64), "claim.basis_exp_sigma")
            counts = band(np.array([b.shape[0] for b in bes], np.uint64), "claim.n")
            gs = band(good["gs"], "claim.g_sigma_neg")
            cl = band(np.array([ptrs.ptr, counts.ptr, gs.ptr], np.uint64), "claim")
            pr, hs, seed = band(np.stack(cer["steps"]), "proofs"), band(np.frombuffer(b"".join(cer["hashes"]), np.uint8), "hashes"), band(np.frombuffer(SEED_B, np.uint8), "seed")
            failed, badc, fb = band(np.full(1, 0xFFFFFFFF, np.uint32), "failed"), band(np.full(1, 77, np.uint64), "bad_commitments"), band(np.full(1, 77, np.uint64), "first_bad_record")
            before = snapshot(ctx, w)
            assert lib.mi_phase2_verify_adopt_sigma(ctx.h, w, cl.arg(), pr.arg(), hs.arg(), C.c_size_t(2), seed.arg(), failed.arg(), badc.arg(), fb.arg()) == 0
            for x in arrays + [ptrs, counts, gs, cl, pr, hs, seed]:
                x.assert_unchanged()
            for x in (failed, badc, fb):
                x.check()
            assert (int(failed.payload(np.uint32)[0]), int(badc.payload()[0]), int(fb.payload()[0])) == want
            if want[0]:
                assert snapshot(ctx, w) == before
        assert ctx.phase2_to_streams(w, T2.RAW) == ctx.phase2_to_streams(p, T2.RAW)
    finally:
        ctx.phase2_free(p); ctx.phase2_free(w)


def test_sigma_results_after_a_larger_call(ctx, ceremony):
    """a call's result is the same after a larger call on the same context: one commitment of one wire, before and after two of 65"""
    B = load_binding()
    cer = ceremony
    r1cs, srs, _, sigma0, sg = inputs(ctx, 1, 1)
    a, a2, b = (ctx.phase2_init(r1cs, srs, sg) for _ in range(3))
    big = ctx.phase2_init(cer["r1cs"], cer["srs"], cer["sg"])
    try:
        step, h = ctx.phase2_contribute_sigma_proved(a, fr_arr(S1[:1]), fr_arr(N1[:1]))
        good = sigma_claim_of(ctx, B, a, 1)
        tampered = dict(good, bes=[ctx.batch_scalar_mul(D.G1, fr_arr([5]))])
        first = adopt_sigma(ctx, b, tampered, [step], [h])
        assert first == (B.PHASE2_BAD_BES, 1, 1)
        # the larger calls: a contribution and an adoption over two commitments of 65 wires
        big_step, big_h = ctx.phase2_contribute_sigma_proved(big, fr_arr(S1), fr_arr(N1))
        assert np.array_equal(big_step, cer["steps"][0]) and big_h == cer["hashes"][0]
        big_claim = sigma_claim_of(ctx, B, big, 2)
        big_claim["bes"][1][64] = big_claim["bes"][1][0]      # a verdict, so that the shared verifier adopts nothing
        before = snapshot(ctx, cer["v"])
        assert adopt_sigma(ctx, cer["v"], big_claim, [big_step], [big_h], SEED_B) == (B.PHASE2_BAD_BES, 2, 1)
        assert snapshot(ctx, cer["v"]) == before
        assert adopt_sigma(ctx, b, tampered, [step], [h]) == first
        step2, h2 = ctx.phase2_contribute_sigma_proved(a2, fr_arr(S1[:1]), fr_arr(N1[:1]))
        assert np.array_equal(step2, step) and h2 == h
        assert adopt_sigma(ctx, b, good, [step], [h]) == (0, 0, 1)
        assert ctx.phase2_to_streams(b, T2.RAW) == ctx.phase2_to_streams(a, T2.RAW)
    finally:
        for s in (a, a2, b, big):
            ctx.phase2_free(s)
