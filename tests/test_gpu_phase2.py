"""GPU: the keys from a powers-of-tau SRS (include/mi355x_groth16_phase2.h, csrc/phase2.hip).  Every comparison is exact.

The yardstick needs no new oracle: phase 2 fixes gamma = 1 and starts at delta = 1, so the key derived from an SRS built with known
(tau, alpha, beta) equals BYTE FOR BYTE the streams mi_groth16_setup_to_streams writes for the trapdoor (tau, alpha, beta, 1, 1, sigma),
and after contributions d_1 .. d_m the streams for delta = d_1 ... d_m (an affine point has one encoding).  The SRS rows are built here
from Python-integer powers through mi_batch_scalar_mul_g1 / _g2.

1  equals Setup at N = 1, 2, 4, a power of two and not one, with and without commitments, both encodings, the sealed vk too
2  independent of Setup: every point of the state against pyref.toy_setup's own double-and-add
3  the complete additions: tau a primitive 2N-th root of unity (tau^N = -1), cancelling entries, a column that cancels to zero,
   a coefficient 0, duplicate columns in a row
4  column lengths at the edges of the cut rule
5  every coefficient path in short and long columns
6  contribute
7  the sealed key is an ordinary key: prove through the pool, verify from bytes
8  refusals
"""
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
import bytes_cases as BC
import verify_cases as V
from helpers import fr_arr, fr_vals, g1_arr, g2_arr, g1_pts, g2_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R = P.R_MOD
RAW, COMPRESSED = 0, 1
FULL = 0x2A3C09F0A58A7E85_00E0A7EB8EF62ABC_402D111E41112ED4_9BD61B6E725B19F1 % R
COEFF_TABLE = [1, R - 1, 2, R - 2, (1 << 32) - 1, 1 << 32, R - (1 << 32), FULL]


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def domain_size(n_constraints):
    return 1 << max(n_constraints - 1, 0).bit_length()


def make_srs(ctx, n_constraints, tau, alpha, beta):
    """the SRS rows for this circuit size from known (tau, alpha, beta): Python-integer powers, the points by the library's fixed-base
    batch scalar multiplication (oracle-checked elsewhere)"""
    N = domain_size(n_constraints)
    pw = [1]
    for _ in range(2 * N - 1):
        pw.append(pw[-1] * tau % R)
    return {"tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr(pw)),
            "alpha_tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr([alpha * p % R for p in pw[:N]])),
            "beta_tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr([beta * p % R for p in pw[:N]])),
            "tau_g2": ctx.batch_scalar_mul(D.G2, fr_arr(pw[:N]), g2=True),
            "beta_g2": ctx.batch_scalar_mul(D.G2, fr_arr([beta]), g2=True)[0]}


def trapdoor(tau, alpha, beta, delta=1, sigma=()):
    td = {n: fr_arr([v])[0] for n, v in (("tau", tau), ("alpha", alpha), ("beta", beta), ("gamma", 1), ("delta", delta))}
    td["sigma"] = [fr_arr([s])[0] for s in sigma]
    return td


def secrets(seed, n_sigma=0):
    rng = P.SplitMix64(seed)
    return rng.fr(), rng.fr(), rng.fr(), [rng.fr() for _ in range(n_sigma)]


def tau_2n_root(n_constraints):
    """a primitive 2N-th root of unity: tau^N = -1, so sums and differences of SRS points cancel"""
    log_n = domain_size(n_constraints).bit_length() - 1
    t = pow(P.FR_ROOT_2_28, 1 << (P.FR_TWO_ADICITY - log_n - 1), R)
    assert pow(t, 1 << log_n, R) == R - 1
    return t


def assert_equals_setup(ctx, r1cs, st, td, encodings=(RAW, COMPRESSED)):
    """the state's two streams against mi_groth16_setup_to_streams's, per encoding; returns Setup's vk dict"""
    vk = None
    for enc in encodings:
        want_pk, want_vk, _, _, vk = ctx.setup_to_streams(r1cs, td, enc, build=False)
        got_pk, got_vk = ctx.phase2_to_streams(st, enc)
        assert got_vk == want_vk, f"verifying key's stream, encoding {enc}"
        assert len(got_pk) == len(want_pk) and got_pk == want_pk, f"proving key's stream, encoding {enc}"
    return vk


def assert_vk_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"vk.{k}"


def free_key(ctx, pkh, peds):
    for pd in peds:
        ctx.pedersen_pk_free(pd)
    ctx.pk_free(pkh)


# ---------------------------------------------------------------------------------------------------- 1: equals Setup
@pytest.mark.parametrize("n_commitments", [0, 2])
@pytest.mark.parametrize("nc", [1, 2, 3, 100, 1000, 4096])
def test_phase2_equals_setup_byte_for_byte(ctx, nc, n_commitments):
    tau, alpha, beta, sigma = secrets(1000 + nc, n_commitments)
    nw = max(48, nc + 40)
    r1cs = S.synth_r1cs(nc, nb_wires=nw, nb_public=5, seed=nc * 10 + n_commitments, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=min(40, nc),
                        n_empty_cols=6, commitments=n_commitments, n_committed=3)
    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, tau, alpha, beta), [fr_arr([s])[0] for s in sigma])
    try:
        stats = ctx.phase2_stats()
        print(f"phase2_init nc = {nc}: {stats}")
        assert stats["entries"] == sum(len(r1cs[m][1]) for m in "ABC")
        want_vk = assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta, 1, sigma))
        pkh, peds, vk = ctx.phase2_seal(st, 5 + n_commitments, n_commitments)
        free_key(ctx, pkh, peds)
        assert_vk_equal(vk, want_vk)
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 2: independent of Setup
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_phase2_state_against_pyref_point_by_point(ctx, nc):
    """every point of the state against pyref.toy_setup's double-and-add over its own exponents (gamma = delta = 1): a mistake shared
    with setup.hip's sort cannot hide here"""
    B = load_binding()
    cs = P.ToyR1CS(nc, 3, 70 + nc, 0.4); td = P.ToyTrapdoor(80 + nc)
    td.gamma = td.delta = 1
    pk, exps, dom = P.toy_setup(cs, td)
    r1cs = S.toy_r1cs(cs)
    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, td.tau, td.alpha, td.beta))
    try:
        assert g1_pts(ctx.phase2_array(st, B.PHASE2_G1_A)) == pk["g1_a"]
        assert g1_pts(ctx.phase2_array(st, B.PHASE2_G1_B)) == pk["g1_b"]
        assert g2_pts(ctx.phase2_array(st, B.PHASE2_G2_B)) == pk["g2_b"]
        assert g1_pts(ctx.phase2_array(st, B.PHASE2_G1_K)) == pk["g1_k"]
        assert g1_pts(ctx.phase2_array(st, B.PHASE2_G1_Z)) == pk["g1_z"]
        assert g1_pts(ctx.phase2_array(st, B.PHASE2_VK_K)) == [P.g1_mul(P.G1_GEN, exps["K"][j]) if exps["K"][j] else None for j in range(cs.nb_public)]
        pkh, peds, vk = ctx.phase2_seal(st, cs.nb_public)
        free_key(ctx, pkh, peds)
        assert g1_pts(vk["alpha1"]) == [pk["alpha1"]] and g2_pts(vk["beta2"]) == [pk["beta2"]]
        assert g2_pts(vk["gamma2"]) == g2_pts(vk["delta2"]) == [P.G2_GEN]
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 3: the complete additions
@pytest.mark.parametrize("nc", [8, 1000])
def test_phase2_tau_a_2n_th_root_of_unity(ctx, nc):
    """tau^N = -1 (mi_groth16_setup accepts it: tau is not on the domain): SRS points that are each other's negatives, so butterflies
    and column sums meet P + (-P) and P - (-P); G1 and G2 are both in the streams"""
    _, alpha, beta, sigma = secrets(3000 + nc, 1)
    tau = tau_2n_root(nc)
    r1cs = S.synth_r1cs(nc, nb_wires=max(48, nc + 40), nb_public=5, seed=31 + nc, per_row=4, n_coeffs=32, n_heavy=2, heavy_len=min(40, nc), n_empty_cols=6,
                        commitments=1, n_committed=3)
    srs = make_srs(ctx, nc, tau, alpha, beta)
    N = domain_size(nc)
    assert np.array_equal(srs["tau_g1"][N][:4], srs["tau_g1"][0][:4]) and not np.array_equal(srs["tau_g1"][N], srs["tau_g1"][0])   # [tau^N]1 = -g1
    st = ctx.phase2_init(r1cs, srs, [fr_arr([sigma[0]])[0]])
    try:
        assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta, 1, sigma))
    finally:
        ctx.phase2_free(st)


def r1cs_from_entries(n_constraints, nb_wires, nb_public, entries, coeff_table):
    """entries: {"A": [(row, col, index into coeff_table)], ...} in any order -> the R1CS dict"""
    out = {"n_constraints": n_constraints, "nb_wires": nb_wires, "nb_public": nb_public, "coeffs": fr_arr(coeff_table), "commitments": []}
    for name in "ABC":
        es = sorted(entries.get(name, []), key=lambda e: e[0])   # stable: the order inside a row is kept
        rp = np.zeros(n_constraints + 1, np.uint64)
        for row, _, _ in es:
            rp[row + 1] += 1
        out[name] = (np.cumsum(rp).astype(np.uint64), np.array([c for _, c, _ in es], np.uint32), np.array([k for _, _, k in es], np.uint32))
    return out


@pytest.mark.parametrize("root_of_unity", [False, True])
def test_phase2_cancelling_entries_and_columns(ctx, root_of_unity):
    """wire 3: c and r - c in one row of A beside another entry (the column sum passes through infinity); wire 4: present in A and B
    with coefficients 6, r - 4, r - 2 in one row (duplicate columns; A_4 = B_4 = 0: the masks must say infinity and the arrays compact
    as Setup's do); wire 5: a coefficient 0 alone; wire 6: the same row twice with equal coefficients (a doubling)"""
    B = load_binding()
    nc, nw = 8, 10
    table = [0, 1, FULL, R - FULL, 6, R - 4, R - 2, 3]
    tau, alpha, beta, _ = secrets(77)
    if root_of_unity:
        tau = tau_2n_root(nc)
    body = [(2, 3, 2), (2, 3, 3), (5, 3, 7), (1, 4, 4), (1, 4, 5), (1, 4, 6), (4, 5, 0), (6, 6, 2), (6, 6, 2), (0, 0, 1), (7, 9, 1), (3, 1, 7)]
    r1cs = r1cs_from_entries(nc, nw, 2, {"A": body, "B": body[3:], "C": [(i, 2 + i, 1) for i in range(8) if i != 3] + [(1, 4, 2)]}, table)
    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, tau, alpha, beta))
    try:
        assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta))
        # wires with a point in A: 0, 1, 3, 6, 9 (4 cancels, 5 has the coefficient 0 alone); in B: 0, 1, 6, 9
        assert len(ctx.phase2_array(st, B.PHASE2_G1_A)) == 5 and len(ctx.phase2_array(st, B.PHASE2_G1_B)) == len(ctx.phase2_array(st, B.PHASE2_G2_B)) == 4
        k = ctx.phase2_array(st, B.PHASE2_G1_K)
        assert len(k) == nw - 2 and k[4 - 2].any() and not k[5 - 2].any()   # t_4 = C's entry alone; wire 5 is in no constraint that counts
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 4: the cut rule's edges
EDGE_LENS = (16, 17, 512, 513, 2 * 512 + 1)


def test_phase2_columns_at_the_split_edges(ctx):
    """columns of exactly 0..4, 16, 17, 512, 513 and 2 * 512 + 1 entries in each matrix (the transposes of r1cs_cases.skewed_r1cs's
    planted rows), for the G1 sums and the G2 sum: a lane's list, the first list cut, one full piece, one piece and one entry, two
    pieces and one entry.  The plan's counts are those of the untransposed rows."""
    src = RC.skewed_r1cs(n_constraints=200, nb_wires=1024, nb_public=9, seed=1408, long_lens=EDGE_LENS, n_coeffs=64)
    r1cs = RC.transposed(src)
    assert r1cs["n_constraints"] == 1024 and r1cs["nb_wires"] == 200
    for name in "ABC":
        lens = np.bincount(r1cs[name][1], minlength=200)
        assert [int(lens[src["long_at"][name][n]]) for n in EDGE_LENS] == list(EDGE_LENS) and set(range(5)) <= set(lens.tolist())
    tau, alpha, beta, _ = secrets(1409)
    st = ctx.phase2_init(r1cs, make_srs(ctx, 1024, tau, alpha, beta))
    try:
        stats = ctx.phase2_stats()
        print(f"phase2_init at the split edges: {stats}")
        assert (stats["long_columns"], stats["chunks"]) == RC.split_counts(src) == (3 * 4, 3 * (1 + 1 + 2 + 3))
        assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta), encodings=(RAW,))
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 5: the coefficient paths
def test_phase2_every_coefficient_path_in_short_and_long_columns(ctx):
    """the table {1, r - 1, 2, r - 2, 2^32 - 1, 2^32, r - 2^32, full width}: an addition, a subtraction, xyzz_mul_u32 on c and on r - c
    at both ends of its range, the full double-and-add.  Wire 3 holds each once (a lane's list), wire 4 forty entries (one piece), wire 5
    seven hundred (two pieces), in every matrix"""
    nc = 700
    body = [(i, 3, i) for i in range(8)] + [(i, 4, i % 8) for i in range(40)] + [(i, 5, (i + 3) % 8) for i in range(700)] + [(0, 0, 0), (9, 1, 7)]
    r1cs = r1cs_from_entries(nc, 8, 2, {"A": body, "B": body[::-1], "C": body[4:]}, COEFF_TABLE)
    tau, alpha, beta, _ = secrets(1510)
    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, tau, alpha, beta))
    try:
        stats = ctx.phase2_stats()
        assert (stats["long_columns"], stats["chunks"]) == (6, 9)
        assert_equals_setup(ctx, r1cs, st, trapdoor(tau, alpha, beta), encodings=(RAW,))
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 6: contribute
def test_phase2_contributions(ctx):
    B = load_binding()
    nc, ncom = 100, 2
    tau, alpha, beta, sigma = secrets(1600, ncom)
    d1, d2, s1a, s1b, s2a, s2b = secrets(1601, 3)[3] + secrets(1602, 3)[3]
    r1cs = S.synth_r1cs(nc, nb_wires=160, nb_public=5, seed=1603, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=ncom, n_committed=4)
    W = cref.gen_scalars(r1cs["nb_wires"], 3, 1); a, b, _ = D.constraint_values(nc, 1, 4); r, s = cref.gen_scalars(2, 5, 0)

    def proves_like_setup(pkh, td):
        """the sealed key's proof equals the proof of the key Setup makes for this trapdoor"""
        ref, ref_peds, _ = ctx.setup(r1cs, td)
        try:
            p1, _ = ctx.prove(pkh, W, a, b, None, r, s)
            p2, _ = ctx.prove(ref, W, a, b, None, r, s)
            assert np.array_equal(p1["raw"], p2["raw"])
        finally:
            free_key(ctx, ref, ref_peds)

    st = ctx.phase2_init(r1cs, make_srs(ctx, nc, tau, alpha, beta), [fr_arr([x])[0] for x in sigma])
    try:
        td0 = trapdoor(tau, alpha, beta, 1, sigma)
        assert_equals_setup(ctx, r1cs, st, td0, encodings=(COMPRESSED,))
        before = ctx.phase2_seal(st, 5 + ncom, ncom)
        try:
            ctx.phase2_contribute(st, fr_arr([d1])[0], fr_arr([s1a, s1b]))
            td1 = trapdoor(tau, alpha, beta, d1, [sigma[0] * s1a % R, sigma[1] * s1b % R])
            assert_equals_setup(ctx, r1cs, st, td1, encodings=(COMPRESSED,))
            ctx.phase2_contribute(st, fr_arr([d2])[0], fr_arr([s2a, s2b]))
            td2 = trapdoor(tau, alpha, beta, d1 * d2 % R, [sigma[0] * s1a * s2a % R, sigma[1] * s1b * s2b % R])
            want_vk = assert_equals_setup(ctx, r1cs, st, td2)
            after = ctx.phase2_seal(st, 5 + ncom, ncom)
            try:
                assert_vk_equal(after[2], want_vk)
                proves_like_setup(before[0], td0)     # sealing did not end the ceremony, and the earlier key still works
                proves_like_setup(after[0], td2)
            finally:
                free_key(ctx, after[0], after[1])
        finally:
            free_key(ctx, before[0], before[1])
        # refusals leave the state as it was
        streams = ctx.phase2_to_streams(st, RAW)
        for delta, sf, word in ((0, [1, 1], "delta"), (5, [1, 0], "sigma_factor[1]")):
            with pytest.raises(B.MiError) as ei:
                ctx.phase2_contribute(st, fr_arr([delta])[0], fr_arr(sf))
            assert "rc=-1:" in str(ei.value) and word in str(ei.value)
            assert ctx.phase2_to_streams(st, RAW) == streams
        # no sigma factors: all 1
        ctx.phase2_contribute(st, fr_arr([7])[0])
        td3 = dict(td2, delta=fr_arr([d1 * d2 * 7 % R])[0])
        assert_equals_setup(ctx, r1cs, st, td3, encodings=(RAW,))
    finally:
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 7: an ordinary key
def test_phase2_sealed_key_proves_and_verifies(ctx):
    """a circuit with a solution and one commitment (the recipe of tests/test_gpu_vkfile.py's round trip): the proof made with the
    sealed key through the prover pool is, byte for byte, the proof made with Setup's key for the same (r, s); the verifier loaded from
    the state's vk stream accepts it from its bytes, the one from before the contribution rejects it at the pairing"""
    B = load_binding()
    ncom, n, nab, nb_public = 1, 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 41, long_lens=(16, 17, 64), commitments=ncom, n_committed=7)
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 42)
    tau, alpha, beta, sigma = secrets(1700, ncom)
    delta = secrets(1701)[0]
    rr, ss = cref.gen_scalars(2, 61, 0)
    st = ctx.phase2_init(r1cs, make_srs(ctx, n, tau, alpha, beta), [fr_arr([sigma[0]])[0]])
    pool = B.Prover(0, 1)
    keys = []
    try:
        _, vk_before = ctx.phase2_to_streams(st, COMPRESSED)
        ctx.phase2_contribute(st, fr_arr([delta])[0])
        _, vk_after = ctx.phase2_to_streams(st, COMPRESSED)
        keys.append(ctx.phase2_seal(st, nb_public + ncom, ncom))
        keys.append(ctx.setup(r1cs, trapdoor(tau, alpha, beta, delta, sigma)))
        (pkh, peds, _), (ref, ref_peds, _) = keys
        pub = fr_vals(W[1:nb_public])
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
        cms = np.stack([pool.commit(peds[k], vals[k]).reshape(8) for k in range(ncom)])
        assert np.array_equal(cms, np.stack([pool.commit(ref_peds[k], vals[k]).reshape(8) for k in range(ncom)]))
        values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
        for (_, cw), v in zip(r1cs["commitments"], values):
            W[cw] = fr_arr([v])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        data = []
        for key, key_peds in ((pkh, peds), (ref, ref_peds)):
            proof, _ = pool.wait(pool.submit_bsb22(key, W, a, b, None, rr, ss, [(key_peds[k], vals[k]) for k in range(ncom)], fr_arr([fold])[0]))
            data.append(B.proof_write(proof["raw"], commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8)))
        assert data[0] == data[1] and len(data[0]) == 196
        for blob, want in ((vk_after, B.VERIFY_OK), (vk_before, B.VERIFY_PAIRING)):
            vkh = ctx.vk_load_stream(blob)
            try:
                assert vkh.verify_bytes(data[0], np.ascontiguousarray(W[1:nb_public])) == want
            finally:
                vkh.free()
    finally:
        pool.close()
        for pkh, peds, _ in keys:
            free_key(ctx, pkh, peds)
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 8: refusals
REFUSAL_NC = 500   # N = 512: two workgroups of the check kernels per row, four for tau_g1


@pytest.fixture(scope="module")
def refusal_inputs(ctx):
    tau, alpha, beta, sigma = secrets(1800, 1)
    r1cs = S.synth_r1cs(REFUSAL_NC, nb_wires=540, nb_public=5, seed=1801, per_row=3, n_coeffs=16, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=1, n_committed=3)
    return r1cs, make_srs(ctx, REFUSAL_NC, tau, alpha, beta), [fr_arr([sigma[0]])[0]]


def _broken(srs, name):
    """name -> (srs, sigma override, flags, the words the message must hold)"""
    srs = dict(srs)
    sigma = None
    if name == "short tau_g1":
        srs["tau_g1"] = srs["tau_g1"][:2 * 512 - 1]
        words = ("srs.n_tau_g1", "1023", "1024")
    elif name == "null row":
        srs["beta_tau_g1"] = None; srs["n_beta_tau_g1"] = 512
        words = ("srs.beta_tau_g1 is null",)
    elif name == "short tau_g2":
        srs["tau_g2"] = srs["tau_g2"][:511]
        words = ("srs.n_tau_g2",)
    elif name == "off-curve G1 point beyond the first workgroup":
        row = srs["alpha_tau_g1"].copy(); row[300, 4] ^= np.uint64(1); row[400, 4] ^= np.uint64(1)   # y of two points: the lowest is named
        srs["alpha_tau_g1"] = row
        words = ("srs.alpha_tau_g1[300]",)
    elif name == "off-curve G1 point in the upper half of tau_g1":
        row = srs["tau_g1"].copy(); row[1023, 0] ^= np.uint64(2)
        srs["tau_g1"] = row
        words = ("srs.tau_g1[1023]",)
    elif name == "G2 point outside the r-torsion":
        row = srs["tau_g2"].copy(); row[301] = g2_arr([V.twist_point_outside_subgroup()])[0]
        srs["tau_g2"] = row
        words = ("srs.tau_g2[301]", "r-torsion")
    elif name == "beta_g2 off the twist":
        b = srs["beta_g2"].copy(); b[8] ^= np.uint64(1)
        srs["beta_g2"] = b
        words = ("srs.beta_g2[0]",)
    elif name == "infinity in a row":
        row = srs["beta_tau_g1"].copy(); row[7] = 0
        srs["beta_tau_g1"] = row
        words = ("srs.beta_tau_g1[7]", "infinity")
    elif name == "infinity in tau_g2":
        row = srs["tau_g2"].copy(); row[0] = 0
        srs["tau_g2"] = row
        words = ("srs.tau_g2[0]", "infinity")
    elif name == "sigma 0":
        sigma = [np.zeros(4, np.uint64)]
        words = ("sigma[0] is 0",)
    else:
        raise KeyError(name)
    return srs, sigma, words


REFUSALS = ("short tau_g1", "null row", "short tau_g2", "off-curve G1 point beyond the first workgroup", "off-curve G1 point in the upper half of tau_g1",
            "G2 point outside the r-torsion", "beta_g2 off the twist", "infinity in a row", "infinity in tau_g2", "sigma 0")


@pytest.mark.parametrize("name", REFUSALS)
def test_phase2_refusals(ctx, refusal_inputs, name):
    B = load_binding()
    r1cs, srs, sigma = refusal_inputs
    ctx.phase2_free(ctx.phase2_init(r1cs, srs, sigma))   # the context's workspaces have their size
    bad_srs, bad_sigma, words = _broken(srs, name)
    before = ctx.mem_ledger()
    with pytest.raises(B.MiError) as ei:
        ctx.phase2_init(r1cs, bad_srs, sigma if bad_sigma is None else bad_sigma)
    assert "rc=-1:" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
    assert ctx.mem_ledger() == before
    if name == "G2 point outside the r-torsion":   # gnark's UnsafeReadFrom: the point is on the twist, so without the test it passes
        ctx.phase2_free(ctx.phase2_init(r1cs, bad_srs, sigma, flags=B.KEYFILE_NO_SUBGROUP_CHECK))
    st = ctx.phase2_init(r1cs, srs, sigma)   # a good init follows
    try:
        assert len(ctx.phase2_array(st, B.PHASE2_G1_Z)) == 512
    finally:
        ctx.phase2_free(st)
    assert ctx.mem_ledger() == before


def test_phase2_refuses_what_setup_refuses_and_null_arguments(ctx, refusal_inputs):
    import ctypes as C
    B = load_binding()
    r1cs, srs, sigma = refusal_inputs
    before = ctx.mem_ledger()
    col_hi = r1cs["B"][1].copy(); col_hi[17] = 540
    for broken, word in ((dict(B=(r1cs["B"][0], col_hi, r1cs["B"][2])), "B.col[17]"), (dict(nb_public=0), "nb_public"), (dict(n_constraints=(1 << 27) + 1), "n_constraints")):
        with pytest.raises(B.MiError) as ei:
            ctx.phase2_init({**r1cs, **broken}, srs, sigma)
        assert "rc=-1:" in str(ei.value) and "phase2" in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(B.MiError, match="unknown flag"):
        ctx.phase2_init(r1cs, srs, sigma, flags=4)
    with pytest.raises(B.MiError, match="sigma is null"):
        ctx.phase2_init(r1cs, srs, [])
    d, keep = B._r1cs_desc(r1cs); sd, keep2 = B._srs_desc(srs); h = C.c_void_p(); sg = np.ascontiguousarray(sigma[0])
    lib = ctx.lib
    assert lib.mi_phase2_init(ctx.h, None, C.byref(sd), B._p(sg), 0, C.byref(h)) == -1
    assert lib.mi_phase2_init(ctx.h, C.byref(d), None, B._p(sg), 0, C.byref(h)) == -1 and b"srs is null" in lib.mi_last_error(ctx.h)
    assert lib.mi_phase2_init(ctx.h, C.byref(d), C.byref(sd), B._p(sg), 0, None) == -1
    assert lib.mi_phase2_init(None, C.byref(d), C.byref(sd), B._p(sg), 0, C.byref(h)) == -1
    assert not h.value
    assert lib.mi_phase2_contribute(ctx.h, None, B._p(sg), None) == -1 and lib.mi_phase2_free(ctx.h, None) == -1
    assert ctx.mem_ledger() == before
