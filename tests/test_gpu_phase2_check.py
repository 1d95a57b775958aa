"""GPU suite: the checks of a ceremony (include/mi355x_groth16_phase2_check.h, csrc/phase2_check.hip): mi_srs_check_powers,
mi_phase2_contribute_proved, mi_phase2_verify_adopt.

Every SRS row and every claimed array is built from KNOWN exponents (Python integers, the points by mi_batch_scalar_mul_g1 / _g2), and
every expected mask is computed IN THE EXPONENT: the test restates r_k with hashlib and evaluates sum_k r_k (x_(k+1) - tau' x_k) and its
kin mod r.  The yardstick shares nothing with the device's MSM and pairing.  A relation whose sum is not 0 must be reported; one whose
sum is 0 must not (the honest terms are 0 identically, so no coefficient enters).  The records of the contributions are restated with
hashlib and oracle/pyref.py's own group law (tests/test_phase2_check_cpu.py's functions)."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import setup_cases as S
import verify_cases as V
import generic_msm_cases as G
import test_gpu_phase2 as T2
import test_phase2_check_cpu as TC
from helpers import fr_arr, fr_vals, g1_arr, g2_arr, g1_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R = P.R_MOD
SEED_A = bytes(range(100, 132))
SEED_B = bytes(range(31, -1, -1))
ROWS = ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2")
MONT = (1 << 256) % R


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def mont_rows(vals):
    """fr_arr for long lists: the Montgomery words of plain integers"""
    return np.frombuffer(b"".join((v * MONT % R).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


def test_mont_rows_is_fr_arr():
    vals = [0, 1, R - 1, T2.FULL, 1 << 200]
    assert np.array_equal(mont_rows(vals), fr_arr(vals))


# ---------------------------------------------------------------------------------------------------- the SRS in the exponent
def honest_exps(N, tau, alpha, beta):
    pw = [1]
    for _ in range(2 * N - 1):
        pw.append(pw[-1] * tau % R)
    return {"tau_g1": pw, "alpha_tau_g1": [alpha * p % R for p in pw[:N]], "beta_tau_g1": [beta * p % R for p in pw[:N]], "tau_g2": pw[:N], "beta_g2": beta}


def srs_points(ctx, exps, base=None):
    """the rows of these exponents; with base = (exponents, rows) only the points that differ from it are computed"""
    out = {}
    for name in ROWS:
        g2 = name == "tau_g2"
        gen = D.G2 if g2 else D.G1
        if base is None:
            out[name] = ctx.batch_scalar_mul(gen, mont_rows(exps[name]), g2=g2)
            continue
        row = base[1][name].copy()
        diff = [k for k, (a, b) in enumerate(zip(exps[name], base[0][name])) if a != b]
        if diff:
            row[diff] = ctx.batch_scalar_mul(gen, mont_rows([exps[name][k] for k in diff]), g2=g2)
        out[name] = row
    out["beta_g2"] = ctx.batch_scalar_mul(D.G2, fr_arr([exps["beta_g2"]]), g2=True)[0]
    return out


def model_mask(B, exps, N, seed):
    """the relations of mi_srs_check_powers in the exponent; r_k is hashed only where a term is not 0"""
    x1, xa, xb, x2, b2 = exps["tau_g1"], exps["alpha_tau_g1"], exps["beta_tau_g1"], exps["tau_g2"], exps["beta_g2"]
    tp = x2[1]

    def powers_defect(x, n):
        acc = 0
        for k in range(n):
            d = (x[k + 1] - tp * x[k]) % R
            if d:
                acc += TC.coeff(seed, k) * d
        return acc % R

    mask = 0
    if x1[0] != 1 or x2[0] != 1:
        mask |= B.SRS_BAD_GENERATORS
    if powers_defect(x1, 2 * N - 1):
        mask |= B.SRS_BAD_TAU_G1
    if powers_defect(xa, N - 1):
        mask |= B.SRS_BAD_ALPHA_G1
    if powers_defect(xb, N - 1):
        mask |= B.SRS_BAD_BETA_G1
    if sum(TC.coeff(seed, k) * (x1[k] - x2[k]) for k in range(N) if x1[k] != x2[k]) % R:
        mask |= B.SRS_BAD_TAU_G2
    if (xb[0] - b2) % R:
        mask |= B.SRS_BAD_BETA_G2
    return mask


# ---------------------------------------------------------------------------------------------------- 1: the coefficients
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ceremony_coefficients_equal_hashlib(ctx, n):
    for seed in (SEED_A, SEED_B):
        assert fr_vals(ctx.ceremony_coeffs(seed, n)) == [TC.coeff(seed, k) for k in range(n)]


# ---------------------------------------------------------------------------------------------------- 2: honest rows
@pytest.mark.parametrize("root_of_unity", [False, True])
@pytest.mark.parametrize("N", [2, 4, 128])
def test_honest_srs_passes(ctx, N, root_of_unity):
    B = load_binding()
    tau, alpha, beta, _ = T2.secrets(5000 + N)
    if root_of_unity:   # [tau^N]1 = -g1: sums of the rows cancel
        tau = T2.tau_2n_root(N)
    exps = honest_exps(N, tau, alpha, beta)
    srs = srs_points(ctx, exps)
    for seed in (SEED_A, SEED_B):
        assert model_mask(B, exps, N, seed) == 0
        assert ctx.srs_check_powers(srs, N, seed) == 0
    assert ctx.srs_check_powers(srs, N, None) == 0   # the operating system's seed
    s = ctx.srs_check_stats()
    print(f"srs check N = {N}: {s}")
    assert s["peak_bytes"] >= 2 * N * 64 and s["total_ms"] > 0


# ---------------------------------------------------------------------------------------------------- 3, 4, 5: one defect, cancelling defects, two seeds
N_DEFECT = 128


@pytest.fixture(scope="module")
def honest128(ctx):
    tau, alpha, beta, _ = T2.secrets(5200)
    exps = honest_exps(N_DEFECT, tau, alpha, beta)
    return exps, srs_points(ctx, exps)


def _defects(B, N):
    """name -> (row, {index: what is added to the exponent}) or a function of the exponents, and the mask the issue states"""
    T1, A, Be, T2_, B2, GEN = B.SRS_BAD_TAU_G1, B.SRS_BAD_ALPHA_G1, B.SRS_BAD_BETA_G1, B.SRS_BAD_TAU_G2, B.SRS_BAD_BETA_G2, B.SRS_BAD_GENERATORS
    return {
        "tau_g1[1]": ("tau_g1", {1: 1}, T1 | T2_),                 # below N: it is one of the points tau_g2 is compared with
        "tau_g1[N]": ("tau_g1", {N: 1}, T1),
        "tau_g1[2N-1]": ("tau_g1", {2 * N - 1: 1}, T1),            # on the shifted side only
        "alpha_tau_g1[0]": ("alpha_tau_g1", {0: 1}, A),
        "alpha_tau_g1[N-1]": ("alpha_tau_g1", {N - 1: 1}, A),
        "beta_tau_g1[0]": ("beta_tau_g1", {0: 1}, Be | B2),
        "tau_g2[1]": ("tau_g2", {1: 1}, T1 | A | Be | T2_),        # redefines tau
        "tau_g2[N-1]": ("tau_g2", {N - 1: 1}, T2_),
        "beta_g2": ("beta_g2", {0: 1}, B2),
        "tau_g1 scaled": ("tau_g1", "scale", GEN | T2_),
        # defects that cancel under EQUAL coefficients: + e at a, - e at b
        "cancelling pair above N": ("tau_g1", {N + 3: 77, N + 40: R - 77}, T1),
        "cancelling pair below N": ("tau_g1", {5: 77, 90: R - 77}, T1 | T2_),
        "cancelling neighbours": ("alpha_tau_g1", {10: 9, 11: R - 9}, A),
    }


DEFECT_NAMES = ("tau_g1[1]", "tau_g1[N]", "tau_g1[2N-1]", "alpha_tau_g1[0]", "alpha_tau_g1[N-1]", "beta_tau_g1[0]", "tau_g2[1]", "tau_g2[N-1]", "beta_g2",
                "tau_g1 scaled", "cancelling pair above N", "cancelling pair below N", "cancelling neighbours")


def _apply(exps, row, change):
    out = {k: (list(v) if isinstance(v, list) else v) for k, v in exps.items()}
    if change == "scale":
        s = 0x1234567 * T2.FULL % R
        out[row] = [s * x % R for x in out[row]]
    elif row == "beta_g2":
        out[row] = (out[row] + change[0]) % R
    else:
        for k, e in change.items():
            out[row][k] = (out[row][k] + e) % R
    return out


@pytest.mark.parametrize("name", DEFECT_NAMES)
def test_one_defect_gives_its_mask(ctx, honest128, name):
    B = load_binding()
    N = N_DEFECT
    row, change, stated = _defects(B, N)[name]
    exps = _apply(honest128[0], row, change)
    srs = srs_points(ctx, exps, honest128)
    for seed in (SEED_A, SEED_B):   # two seeds, the same masks
        assert model_mask(B, exps, N, seed) == stated, "the model in the exponent against the stated mask"
        assert ctx.srs_check_powers(srs, N, seed) == stated
    if name.startswith("cancelling"):   # the sums DO cancel when every coefficient is the same: what equal coefficients would miss
        x, tp = exps[row], exps["tau_g2"][1]
        assert sum(x[k + 1] - tp * x[k] for k in range(len(x) - 1)) % R == 0


# ---------------------------------------------------------------------------------------------------- 6: past the MSM's sort switch
def test_defect_past_the_sort_switch(ctx):
    """N = 2^18: the tau_g1 MSMs have 2^19 - 1 terms, above the size at which a c = 16 MSM takes the two-pass sort.  The MSM's own plan
    gives c = 15 below 2^20 pairs and with it the one-pass sort, so the case runs twice: as the library runs it, and with c = 16 set
    through the plan knob, where the counter shows that the two-pass sort ran.  The only large case."""
    B = load_binding()
    N = 1 << 18
    assert 2 * N - 1 > G.SORT_SWITCH
    tau, alpha, beta, _ = T2.secrets(5300)
    exps = honest_exps(N, tau, alpha, beta)
    exps["tau_g1"][2 * N - 1] = (exps["tau_g1"][2 * N - 1] + 1) % R
    srs = srs_points(ctx, exps)
    assert model_mask(B, exps, N, SEED_A) == B.SRS_BAD_TAU_G1
    assert ctx.srs_check_powers(srs, N, SEED_A) == B.SRS_BAD_TAU_G1
    print(f"srs check N = 2^18: {ctx.srs_check_stats()}")
    sorts = ctx.counter("generic_sorts_two_pass")
    try:
        assert ctx.lib.mi_debug_set_msm_plan(ctx.h, 16, 0, 0, 0, 0) == 0
        assert ctx.srs_check_powers(srs, N, SEED_A) == B.SRS_BAD_TAU_G1
    finally:
        assert ctx.lib.mi_debug_set_msm_plan(ctx.h, 0, 0, 0, 0, 0) == 0
    assert ctx.counter("generic_sorts_two_pass") >= sorts + 3, "the three MSMs over tau_g1 (2^19 - 1, 2^19 - 1 and 2^18 terms) took the two-pass sort"


# ---------------------------------------------------------------------------------------------------- 7: refusals
@pytest.fixture(scope="module")
def refusal_inputs(ctx):
    """the circuit and the SRS of test_gpu_phase2.py's refusal set"""
    tau, alpha, beta, sigma = T2.secrets(1800, 1)
    r1cs = S.synth_r1cs(T2.REFUSAL_NC, nb_wires=540, nb_public=5, seed=1801, per_row=3, n_coeffs=16, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=1, n_committed=3)
    return r1cs, T2.make_srs(ctx, T2.REFUSAL_NC, tau, alpha, beta), [fr_arr([sigma[0]])[0]]


@pytest.mark.parametrize("name", [n for n in T2.REFUSALS if n != "sigma 0"])
def test_srs_check_refuses_what_init_refuses(ctx, refusal_inputs, name):
    B = load_binding()
    r1cs, srs, sigma = refusal_inputs
    assert ctx.srs_check_powers(srs, 512, SEED_A) == 0   # the context's workspaces have their size
    bad_srs, _, words = T2._broken(srs, name)
    with pytest.raises(B.MiError) as init_err:
        ctx.phase2_init(r1cs, bad_srs, sigma)
    before = ctx.mem_ledger()
    with pytest.raises(B.MiError) as ei:
        ctx.srs_check_powers(bad_srs, 512, SEED_A)
    assert str(ei.value) == str(init_err.value) and "rc=-1:" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
    assert ctx.mem_ledger() == before
    if name == "G2 point outside the r-torsion":   # the flag is honoured: the point is on the twist, the call reaches a verdict
        assert isinstance(ctx.srs_check_powers(bad_srs, 512, SEED_A, flags=B.KEYFILE_NO_SUBGROUP_CHECK), int)
    assert ctx.srs_check_powers(srs, 512, SEED_A) == 0   # a good call follows
    assert ctx.mem_ledger() == before


def test_srs_check_refuses_bad_sizes_and_null_arguments(ctx, refusal_inputs):
    B = load_binding()
    _, srs, _ = refusal_inputs
    before = ctx.mem_ledger()
    for n in (0, 1, 3, 1 << 28):
        with pytest.raises(B.MiError, match="n_domain"):
            ctx.srs_check_powers(srs, n, SEED_A)
    with pytest.raises(B.MiError, match="srs.n_tau_g1"):
        ctx.srs_check_powers(srs, 1024, SEED_A)   # the rows are for N = 512
    with pytest.raises(B.MiError, match="unknown flag"):
        ctx.srs_check_powers(srs, 512, SEED_A, flags=4)
    sd, keep = B._srs_desc(srs); failed = C.c_uint32(7); lib = ctx.lib
    assert lib.mi_srs_check_powers(None, C.byref(sd), C.c_uint64(512), SEED_A, 0, C.byref(failed)) == -1
    assert lib.mi_srs_check_powers(ctx.h, None, C.c_uint64(512), SEED_A, 0, C.byref(failed)) == -1 and b"srs is null" in lib.mi_last_error(ctx.h)
    assert lib.mi_srs_check_powers(ctx.h, C.byref(sd), C.c_uint64(512), SEED_A, 0, None) == -1
    assert lib.mi_srs_check_get_stats(ctx.h, None) == -1 and lib.mi_debug_ceremony_coeffs_dev(ctx.h, None, C.c_size_t(4), None) == -1
    assert failed.value == 7 and ctx.mem_ledger() == before


# ---------------------------------------------------------------------------------------------------- 8, 9, 10: contributions
NC = 100           # the circuit of test_gpu_phase2.py's test_phase2_contributions: N = 128
D1, D2 = T2.secrets(1601, 3)[3][0], T2.secrets(1602, 3)[3][0]
K1, K2 = T2.secrets(1611, 2)[3]


def circuit(ncom):
    return S.synth_r1cs(NC, nb_wires=160, nb_public=5, seed=1603, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=ncom, n_committed=4)


def record_tuple(rec):
    return g1_pts(rec[:8])[0], g1_pts(rec[8:16])[0], fr_vals(rec[16:20])[0], rec[20:].tobytes()


def records_first_bad(start, start_hash, first_index, recs):
    """mi_phase2_records_verify restated: hashlib and pyref's group law"""
    before, prev = start, start_hash
    for i, rec in enumerate(recs):
        after, commit, z, h = record_tuple(rec)
        if h != TC.record_hash(prev, first_index + i, before, after, commit):
            return i
        if P.g1_mul(before, z) != P.g1_add(commit, P.g1_mul(after, TC.challenge(h))):
            return i
        before, prev = after, h
    return len(recs)


def claim_of(ctx, B, st, delta):
    """what a contributor hands over: the state's Z and K, delta1 and delta2 for the product of the contributions so far"""
    return {"g1_z": ctx.phase2_array(st, B.PHASE2_G1_Z), "g1_k": ctx.phase2_array(st, B.PHASE2_G1_K),
            "delta1": ctx.batch_scalar_mul(D.G1, fr_arr([delta]))[0], "delta2": ctx.batch_scalar_mul(D.G2, fr_arr([delta]), g2=True)[0]}


def adopt(ctx, st, claim, records, seed=SEED_A):
    return ctx.phase2_verify_adopt(st, claim["g1_z"], claim["g1_k"], claim["delta1"], claim["delta2"], np.stack(records), seed)


@pytest.mark.parametrize("ncom", [0, 2])
def test_proved_contributions_are_adopted(ctx, ncom):
    B = load_binding()
    tau, alpha, beta, sigma = T2.secrets(1600, ncom)
    r1cs = circuit(ncom)
    srs = T2.make_srs(ctx, NC, tau, alpha, beta)
    sg = [fr_arr([x])[0] for x in sigma]
    states = [ctx.phase2_init(r1cs, srs, sg) for _ in range(3)]
    st, v_all, v_step = states
    try:
        rec1 = ctx.phase2_contribute_proved(st, fr_arr([D1])[0], fr_arr([K1])[0])
        claim1 = claim_of(ctx, B, st, D1)
        rec2 = ctx.phase2_contribute_proved(st, fr_arr([D2])[0], fr_arr([K2])[0])
        claim2 = claim_of(ctx, B, st, D1 * D2 % R)
        # the records are reproducible: the restatement from the exponents, with pyref's points
        want = TC.records_array(TC.chain(TC.ID0, 0, 1, [(D1, K1), (D2, K2)]))
        assert np.array_equal(np.stack([rec1, rec2]), want)
        assert np.array_equal(rec2[:8], claim2["delta1"]) and B.phase2_records_verify(D.G1, TC.ID0, 0, want) == 2
        # the arrays are what mi_phase2_contribute makes of them: Setup's key for delta = d1 d2, sigma as it was (BasisExpSigma is left alone)
        td = T2.trapdoor(tau, alpha, beta, D1 * D2 % R, sigma)
        T2.assert_equals_setup(ctx, r1cs, st, td, encodings=(T2.COMPRESSED,))
        streams = ctx.phase2_to_streams(st, T2.COMPRESSED)
        # both records at once
        assert adopt(ctx, v_all, claim2, [rec1, rec2]) == (0, 2)
        assert ctx.phase2_to_streams(v_all, T2.COMPRESSED) == streams
        T2.assert_equals_setup(ctx, r1cs, v_all, td, encodings=(T2.RAW,))
        print(f"verify_adopt nc = {NC}: {ctx.srs_check_stats(verify=True)}")
        # one record at a time; the second does not verify before the first is adopted
        before = ctx.phase2_to_streams(v_step, T2.RAW)
        mask, fb = adopt(ctx, v_step, claim2, [rec2])
        assert mask & B.PHASE2_BAD_RECORD and fb == 0 and ctx.phase2_to_streams(v_step, T2.RAW) == before
        assert adopt(ctx, v_step, claim1, [rec1]) == (0, 1)
        T2.assert_equals_setup(ctx, r1cs, v_step, T2.trapdoor(tau, alpha, beta, D1, sigma), encodings=(T2.COMPRESSED,))
        assert adopt(ctx, v_step, claim2, [rec2], seed=None) == (0, 1)
        assert ctx.phase2_to_streams(v_step, T2.COMPRESSED) == streams
        # the adopted chain goes on: a third contribution on the adopter verifies for the contributor's own state
        d3, k3 = T2.secrets(1612, 2)[3]
        rec3 = ctx.phase2_contribute_proved(v_step, fr_arr([d3])[0], fr_arr([k3])[0])
        assert np.array_equal(rec3, TC.records_array(TC.chain(rec2[20:].tobytes(), 2, D1 * D2 % R, [(d3, k3)]))[0])
        assert adopt(ctx, st, claim_of(ctx, B, v_step, D1 * D2 * d3 % R), [rec3]) == (0, 1)
        assert ctx.phase2_to_streams(st, T2.RAW) == ctx.phase2_to_streams(v_step, T2.RAW)
        # a nonce from the operating system: the record holds all the same
        rec4 = ctx.phase2_contribute_proved(st, fr_arr([5])[0])
        assert B.phase2_records_verify(rec3[:8], rec3[20:].tobytes(), 3, rec4) == 1
    finally:
        for s in states:
            ctx.phase2_free(s)


# ---- tampers, with every exponent known (no commitments)
def circuit_exponents(r1cs, tau, alpha, beta):
    """Z (bit-reversed) and the private wires' K of the state after mi_phase2_init, in the exponent"""
    N = T2.domain_size(r1cs["n_constraints"]); log_n = N.bit_length() - 1
    L = P.lagrange_at(P.Domain(N), tau)
    coeffs = fr_vals(r1cs["coeffs"])
    t = [0] * r1cs["nb_wires"]
    for name, factor in (("A", beta), ("B", alpha), ("C", 1)):
        row_ptr, col, cf = r1cs[name]
        for i in range(r1cs["n_constraints"]):
            for e in range(int(row_ptr[i]), int(row_ptr[i + 1])):
                t[int(col[e])] = (t[int(col[e])] + coeffs[int(cf[e])] * factor * L[i]) % R
    z = [0] * N
    for i in range(N):
        z[int(format(i, f"0{log_n}b")[::-1], 2)] = (pow(tau, i + N, R) - pow(tau, i, R)) % R
    return z, t[r1cs["nb_public"]:]


@pytest.fixture(scope="module")
def ceremony(ctx):
    """a contributor's state after two proved contributions, its claim from the exponents, and a verifier's fresh state"""
    B = load_binding()
    tau, alpha, beta, _ = T2.secrets(1600)
    r1cs = circuit(0)
    srs = T2.make_srs(ctx, NC, tau, alpha, beta)
    st, v = ctx.phase2_init(r1cs, srs), ctx.phase2_init(r1cs, srs)
    recs = [ctx.phase2_contribute_proved(st, fr_arr([D1])[0], fr_arr([K1])[0]), ctx.phase2_contribute_proved(st, fr_arr([D2])[0], fr_arr([K2])[0])]
    z, k = circuit_exponents(r1cs, tau, alpha, beta)
    yield {"r1cs": r1cs, "srs": srs, "st": st, "v": v, "recs": recs, "z": z, "k": k, "delta": D1 * D2 % R, "trapdoor": (tau, alpha, beta)}
    ctx.phase2_free(st); ctx.phase2_free(v)


def claim_from_exponents(ctx, z, k, e1, e2):
    return {"g1_z": ctx.batch_scalar_mul(D.G1, fr_arr(z)), "g1_k": ctx.batch_scalar_mul(D.G1, fr_arr(k)),
            "delta1": ctx.batch_scalar_mul(D.G1, fr_arr([e1]))[0], "delta2": ctx.batch_scalar_mul(D.G2, fr_arr([e2]), g2=True)[0]}


def adopt_model(B, cer, z_claim, k_claim, e1, e2, recs, seed, start_hash=TC.ID0):
    """mi_phase2_verify_adopt for the verifier's fresh state (delta = 1, no record yet) in the exponent"""
    mask = 0
    fb = records_first_bad(P.G1_GEN, start_hash, 0, recs)
    if fb != len(recs):
        mask |= B.PHASE2_BAD_RECORD
    if record_tuple(recs[-1])[0] != P.g1_mul(P.G1_GEN, e1) or e1 != e2:
        mask |= B.PHASE2_BAD_DELTA
    if sum(TC.coeff(seed, i) * (zc * e2 - zo) for i, (zc, zo) in enumerate(zip(z_claim, cer["z"]))) % R:
        mask |= B.PHASE2_BAD_Z
    if sum(TC.coeff(seed, i) * (kc * e2 - ko) for i, (kc, ko) in enumerate(zip(k_claim, cer["k"]))) % R:
        mask |= B.PHASE2_BAD_K
    return mask, fb


def test_the_exponents_are_the_states(ctx, ceremony):
    """the model's Z and K are the verifier's arrays, and divided by delta the contributor's (zero exponents are points at infinity)"""
    B = load_binding()
    cer = ceremony
    inv = P.fr_inv(cer["delta"])
    fresh = claim_from_exponents(ctx, cer["z"], cer["k"], 1, 1)
    assert np.array_equal(fresh["g1_z"], ctx.phase2_array(cer["v"], B.PHASE2_G1_Z)) and np.array_equal(fresh["g1_k"], ctx.phase2_array(cer["v"], B.PHASE2_G1_K))
    assert 0 in cer["k"] and not fresh["g1_k"][cer["k"].index(0)].any(), "the circuit's empty columns: (0, 0) inside K"
    honest = claim_from_exponents(ctx, [x * inv % R for x in cer["z"]], [x * inv % R for x in cer["k"]], cer["delta"], cer["delta"])
    mine = claim_of(ctx, B, cer["st"], cer["delta"])
    assert all(np.array_equal(honest[n], mine[n]) for n in honest)


def _tampers(B, cer):
    """name -> (claimed Z exponents, claimed K exponents, delta1's, delta2's, the records, the stated mask, first_bad_record)"""
    d, inv = cer["delta"], P.fr_inv(cer["delta"])
    z = [x * inv % R for x in cer["z"]]; k = [x * inv % R for x in cer["k"]]
    recs = cer["recs"]
    last_k = max(i for i, x in enumerate(k) if x)

    def bump(lst, i):
        out = list(lst); out[i] = (out[i] + 1) % R
        return out
    wrong_z = recs[1].copy(); wrong_z[16:20] = fr_arr([(fr_vals(recs[1][16:20])[0] + 1) % R])[0]
    other_id = [np.asarray(r) for r in TC.records_array(TC.chain(TC.ID1, 0, 1, [(D1, K1), (D2, K2)]))]
    inv3 = P.fr_inv(d * 3 % R)
    return {
        "K[0]": (z, bump(k, 0), d, d, recs, B.PHASE2_BAD_K, 2),
        "K[last]": (z, bump(k, last_k), d, d, recs, B.PHASE2_BAD_K, 2),
        "Z[0]": (bump(z, 0), k, d, d, recs, B.PHASE2_BAD_Z, 2),
        "Z[N-1]": (bump(z, len(z) - 1), k, d, d, recs, B.PHASE2_BAD_Z, 2),
        "Z scaled by another factor than K": ([x * inv3 % R for x in cer["z"]], k, d, d, recs, B.PHASE2_BAD_Z, 2),
        "delta2 of another delta": (z, k, d, (d + 1) % R, recs, B.PHASE2_BAD_DELTA | B.PHASE2_BAD_Z | B.PHASE2_BAD_K, 2),
        "delta1 that is not the last record's": (z, k, (d + 1) % R, d, recs, B.PHASE2_BAD_DELTA, 2),
        "a wrong response": (z, k, d, d, [recs[0], wrong_z], B.PHASE2_BAD_RECORD, 1),
        "records of another transcript id": (z, k, d, d, other_id, B.PHASE2_BAD_RECORD, 0),
    }


TAMPER_NAMES = ("K[0]", "K[last]", "Z[0]", "Z[N-1]", "Z scaled by another factor than K", "delta2 of another delta", "delta1 that is not the last record's",
                "a wrong response", "records of another transcript id")


@pytest.mark.parametrize("name", TAMPER_NAMES)
def test_a_tampered_claim_gives_its_bit(ctx, ceremony, name):
    B = load_binding()
    cer = ceremony
    z, k, e1, e2, recs, stated, first_bad = _tampers(B, cer)[name]
    claim = claim_from_exponents(ctx, z, k, e1, e2)
    before = ctx.phase2_to_streams(cer["v"], T2.RAW)
    for seed in (SEED_A, SEED_B):
        assert adopt_model(B, cer, z, k, e1, e2, recs, seed) == (stated, first_bad), "the model in the exponent against the stated mask"
        assert adopt(ctx, cer["v"], claim, recs, seed) == (stated, first_bad)
        assert ctx.phase2_to_streams(cer["v"], T2.RAW) == before


def test_a_state_advanced_without_a_record_does_not_verify(ctx, ceremony):
    """plain mi_phase2_contribute moves delta1 and leaves the chain where it was: the next record starts from a point nobody else has"""
    B = load_binding()
    cer = ceremony
    p = ctx.phase2_init(cer["r1cs"], cer["srs"])
    try:
        ctx.phase2_contribute(p, fr_arr([D1])[0])
        rec = ctx.phase2_contribute_proved(p, fr_arr([D2])[0], fr_arr([K2])[0])
        assert np.array_equal(rec, TC.records_array(TC.chain(TC.ID0, 0, D1, [(D2, K2)]))[0])   # index 0, from [d1]1
        inv = P.fr_inv(cer["delta"])
        z = [x * inv % R for x in cer["z"]]; k = [x * inv % R for x in cer["k"]]
        want = adopt_model(B, cer, z, k, cer["delta"], cer["delta"], [rec], SEED_A)
        assert want == (B.PHASE2_BAD_RECORD, 0)
        before = ctx.phase2_to_streams(cer["v"], T2.RAW)
        assert adopt(ctx, cer["v"], claim_of(ctx, B, p, cer["delta"]), [rec]) == want
        assert ctx.phase2_to_streams(cer["v"], T2.RAW) == before
    finally:
        ctx.phase2_free(p)


def test_transcript_id(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    a, b = ctx.phase2_init(cer["r1cs"], cer["srs"]), ctx.phase2_init(cer["r1cs"], cer["srs"])
    try:
        ctx.phase2_set_transcript_id(a, TC.ID1)
        ctx.phase2_set_transcript_id(a, TC.ID0); ctx.phase2_set_transcript_id(a, TC.ID1)   # any number of times before the first record
        recs = [ctx.phase2_contribute_proved(a, fr_arr([D1])[0], fr_arr([K1])[0]), ctx.phase2_contribute_proved(a, fr_arr([D2])[0], fr_arr([K2])[0])]
        assert np.array_equal(np.stack(recs), TC.records_array(TC.chain(TC.ID1, 0, 1, [(D1, K1), (D2, K2)])))
        with pytest.raises(B.MiError, match="transcript id"):
            ctx.phase2_set_transcript_id(a, TC.ID0)
        claim = claim_of(ctx, B, a, cer["delta"])
        mask, fb = adopt(ctx, b, claim, recs)      # b's chain starts from the zero id
        assert (mask, fb) == (B.PHASE2_BAD_RECORD, 0)
        ctx.phase2_set_transcript_id(b, TC.ID1)
        assert adopt(ctx, b, claim, recs) == (0, 2)
        with pytest.raises(B.MiError, match="transcript id"):   # an adopted record counts
            ctx.phase2_set_transcript_id(b, TC.ID1)
        assert ctx.phase2_to_streams(b, T2.RAW) == ctx.phase2_to_streams(a, T2.RAW)
    finally:
        ctx.phase2_free(a); ctx.phase2_free(b)


def test_adopt_and_contribute_proved_refusals_leave_the_state_alone(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    recs = cer["recs"]
    v = ctx.phase2_init(cer["r1cs"], cer["srs"])   # a verifier of its own: this test ends by adopting
    try:
        _refusals(ctx, B, cer, v, recs)
    finally:
        ctx.phase2_free(v)


def _refusals(ctx, B, cer, v, recs):
    good = claim_of(ctx, B, cer["st"], cer["delta"])
    before = ctx.phase2_to_streams(v, T2.RAW)
    ledger = ctx.mem_ledger()

    def refused(claim, records, *words):
        with pytest.raises(B.MiError) as ei:
            adopt(ctx, v, claim, records)
        assert "rc=-1:" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
        assert ctx.phase2_to_streams(v, T2.RAW) == before and ctx.mem_ledger() == ledger
    refused(dict(good, g1_z=good["g1_z"][:-1]), recs, "claim.n_z", "127", "128")
    refused(dict(good, g1_k=good["g1_k"][:-1]), recs, "claim.n_k")
    off = good["g1_z"].copy(); off[70, 4] ^= np.uint64(1); off[90, 4] ^= np.uint64(1)
    refused(dict(good, g1_z=off), recs, "claim.g1_z[70]")
    off = good["g1_k"].copy(); off[3, 0] ^= np.uint64(2)
    refused(dict(good, g1_k=off), recs, "claim.g1_k[3]")
    refused(dict(good, delta2=g2_arr([V.twist_point_outside_subgroup()])[0]), recs, "claim.delta2", "r-torsion")
    off = good["delta2"].copy(); off[8] ^= np.uint64(1)
    refused(dict(good, delta2=off), recs, "claim.delta2", "not on its curve")
    refused(dict(good, delta1=np.zeros(8, np.uint64)), recs, "claim.delta1", "infinity")
    refused(dict(good, delta2=np.zeros(16, np.uint64)), recs, "claim.delta2", "infinity")
    with pytest.raises(B.MiError, match="m is 0"):
        ctx.phase2_verify_adopt(v, good["g1_z"], good["g1_k"], good["delta1"], good["delta2"], np.zeros((0, 24), np.uint64), SEED_A)
    lib = ctx.lib
    failed = C.c_uint32(7)
    assert lib.mi_phase2_verify_adopt(ctx.h, None, None, None, C.c_size_t(1), SEED_A, C.byref(failed), None) == -1
    assert lib.mi_phase2_verify_adopt(ctx.h, v, None, B._p(np.stack(recs)), C.c_size_t(2), SEED_A, C.byref(failed), None) == -1 and failed.value == 7
    # mi_phase2_contribute_proved: delta or nonce 0, a nonce that is not below r
    p = ctx.phase2_init(cer["r1cs"], cer["srs"])
    try:
        p_before = ctx.phase2_to_streams(p, T2.RAW)
        for delta, nonce, word in ((0, K1, "delta is 0"), (D1, 0, "nonce is 0")):
            with pytest.raises(B.MiError, match=word):
                ctx.phase2_contribute_proved(p, fr_arr([delta])[0], fr_arr([nonce])[0])
        with pytest.raises(B.MiError, match="nonce is not below r"):
            ctx.phase2_contribute_proved(p, fr_arr([D1])[0], np.frombuffer(R.to_bytes(32, "little"), np.uint64))
        assert lib.mi_phase2_contribute_proved(ctx.h, p, B._p(fr_arr([D1])[0]), None, None) == -1
        assert ctx.phase2_to_streams(p, T2.RAW) == p_before
        # the chain did not move either: the state's first record is record 0 of the zero id
        rec = ctx.phase2_contribute_proved(p, fr_arr([D1])[0], fr_arr([K1])[0])
        assert np.array_equal(rec, recs[0])
    finally:
        ctx.phase2_free(p)
    # and the verifier's state, untouched through all of it, still adopts the honest claim
    assert ctx.phase2_to_streams(v, T2.RAW) == before
    assert adopt(ctx, v, good, recs) == (0, 2)
    assert ctx.phase2_to_streams(v, T2.RAW) == ctx.phase2_to_streams(cer["st"], T2.RAW)
