"""GPU: groth16.Setup on the device (include/mi355x_groth16_setup.h, csrc/setup.hip).  Every comparison is exact.

1  against the definition: pyref.ToyR1CS circuits, exponents entry for entry against pyref.toy_setup, a proof from the device-made key
   byte-identical to the oracle's proof on toy_setup's key, pyref.trapdoor_check, the verifying key's points
2  skew and size: seeded synthetic R1CS at 2^16 and 2^20 constraints (tests/setup_cases.py) against a host reference built from
   cref.field_op and Python integers
3  a whole key at the benchmark's shape (log_n = 23, one commitment over N / 32 wires), checked through its exponents and through
   proofs in the exponent (tests/dlog_keys.py)
4  refusals: MI_EINVAL on the host, the message names the field, the memory ledger does not move
5  a setup-made key is an ordinary key: table plan, ledger, free, trim
"""
import time
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
from helpers import fr_arr, fr_vals, g1_arr, g2_arr, g1_pts, g2_pts, toy_pk_arrays
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- 1: against the definition
def _toy_setup_exps_only(cs, td):
    """pyref.toy_setup's exponents without its double-and-add over every point (minutes in Python above a few hundred wires): the
    point multiplications are stubbed out for the call, the exponents are toy_setup's own"""
    g1, g2 = P.g1_mul, P.g2_mul
    P.g1_mul = P.g2_mul = lambda p, k: None
    try:
        pk, exps, dom = P.toy_setup(cs, td)
    finally:
        P.g1_mul, P.g2_mul = g1, g2
    return pk, exps, dom


def _toy_key_from_exps(cs, td, pk, exps):
    """toy_setup's key from toy_setup's exponents, the points by the oracle's batch scalar multiplication (oracle/groth16_ref.c)"""
    A, B, K, Z = (fr_arr(exps[k]) for k in "ABKZ")
    ia, ib = np.array(pk["inf_a"]), np.array(pk["inf_b"])
    sm = lambda sc, g2=False: cref.batch_scalar_mul(D.G2 if g2 else D.G1, np.ascontiguousarray(sc).reshape(-1, 4), g2=g2)
    tdv = {k: fr_arr([getattr(td, k)]) for k in ("alpha", "beta", "delta")}
    return {"log_n": pk["log_n"], "nb_public": pk["nb_public"], "nb_wires": pk["nb_wires"],
            "g1_a": sm(A[~ia]), "g1_b": sm(B[~ib]), "g2_b": sm(B[~ib], True), "g1_k": sm(K[cs.nb_public:]),
            "g1_z": sm(Z[D.bitrev_index(pk["log_n"])]),
            "alpha1": sm(tdv["alpha"])[0], "beta1": sm(tdv["beta"])[0], "delta1": sm(tdv["delta"])[0],
            "beta2": sm(tdv["beta"], True)[0], "delta2": sm(tdv["delta"], True)[0],
            "infinity_a": ia.astype(np.uint8), "infinity_b": ib.astype(np.uint8)}


@pytest.mark.parametrize("small_frac", [0.0, 0.9])
@pytest.mark.parametrize("nc", [100, 1000, 4096])
def test_setup_against_the_definition(ctx, nc, small_frac):
    B = load_binding()
    seed = nc + int(small_frac * 10)
    cs = P.ToyR1CS(nc, 5, seed, small_frac); td = P.ToyTrapdoor(seed)
    if nc <= 100:
        pk, exps, dom = P.toy_setup(cs, td)       # the whole definition, points included
        pk_arrays = toy_pk_arrays(pk)
    else:
        pk, exps, dom = _toy_setup_exps_only(cs, td)
        pk_arrays = _toy_key_from_exps(cs, td, pk, exps)
    r1cs, tdd = S.toy_r1cs(cs), S.toy_trapdoor(td)
    got = ctx.setup_exponents(r1cs, tdd)
    for key, name in (("a", "A"), ("b", "B"), ("c", "C"), ("k", "K")):
        assert fr_vals(got[key]) == exps[name], f"{name} exponents"
    assert fr_vals(got["z"]) == P.bit_reverse_perm(exps["Z"]), "Z exponents (stored order)"
    assert list(got["infinity_a"]) == [int(x) for x in pk["inf_a"]] and list(got["infinity_b"]) == [int(x) for x in pk["inf_b"]]
    # the key, through a proof
    w, a, b, c = cs.solve()
    rng = P.SplitMix64(seed + 1); r, s = rng.fr(), rng.fr()
    W, av, bv, cv, rv, sv = fr_arr(w), fr_arr(a), fr_arr(b), fr_arr(c), fr_arr([r])[0], fr_arr([s])[0]
    pkh, peds, vk = ctx.setup(r1cs, tdd)
    try:
        proof, _ = ctx.prove(pkh, W, av, bv, cv, rv, sv)
    finally:
        ctx.pk_free(pkh)
    assert peds == []
    want, h = cref.prove(pk_arrays, W, av, bv, cv, rv, sv, want_h=True)
    assert B.proof_write(proof["raw"]) == cref.proof_write(want["raw"])
    chk = {"ar": g1_pts(proof["ar"])[0], "bs": g2_pts(proof["bs"])[0], "krs": g1_pts(proof["krs"])[0], "h": fr_vals(h)}
    assert P.trapdoor_check(cs, td, exps, chk, r, s)
    # the verifying key
    R = P.R_MOD
    assert g1_pts(vk["alpha1"]) == [P.g1_mul(P.G1_GEN, td.alpha)]
    assert g2_pts(vk["beta2"]) == [P.g2_mul(P.G2_GEN, td.beta)] and g2_pts(vk["gamma2"]) == [P.g2_mul(P.G2_GEN, td.gamma)]
    assert g2_pts(vk["delta2"]) == [P.g2_mul(P.G2_GEN, td.delta)]
    ginv = P.fr_inv(td.gamma)
    want_k = [P.g1_mul(P.G1_GEN, (td.beta * exps["A"][j] + td.alpha * exps["B"][j] + exps["C"][j]) * ginv % R) for j in range(cs.nb_public)]
    assert g1_pts(vk["k"]) == want_k


# ---------------------------------------------------------------------------------------------------- 2: skew and size
@pytest.mark.parametrize("log_n,n_coeffs", [(16, 1), (16, 1 << 16), (20, 1 << 16)])
def test_setup_exponents_skew_and_size(ctx, log_n, n_coeffs):
    n = (1 << log_n) - 1234                               # not a power of two
    r1cs = S.synth_r1cs(n, nb_wires=(1 << log_n) + 777, nb_public=33, seed=log_n * 100 + (n_coeffs > 1), per_row=4, n_coeffs=n_coeffs,
                        n_heavy=200 if log_n == 20 else 24)
    td = S.synth_trapdoor(log_n + 5)
    t0 = time.perf_counter()
    got = ctx.setup_exponents(r1cs, td)
    st = ctx.setup_stats()
    print(f"setup_exponents 2^{log_n}: {time.perf_counter() - t0:.2f} s wall; {st}")
    assert st["entries"] == 3 * len(r1cs["A"][1]) and st["long_columns"] >= 2 and st["chunks"] > st["long_columns"]
    t0 = time.perf_counter()
    S.check_exponents(r1cs, td, got, seed=log_n)
    S.check_z(td, log_n, got["z"])
    print(f"host reference 2^{log_n}: {time.perf_counter() - t0:.1f} s on {cref.num_threads()} threads")


def test_setup_columns_at_the_split_edges(ctx):
    """Columns of exactly 0..4, 16, 17, 64, 511, 512, 513, 5000 and 100 003 entries (r1cs_cases.LONG_LENS: the last is 196 pieces, so the
    combine pass's lane stride loops): the transposes of r1cs_cases.skewed_r1cs's matrices, whose planted ROWS those are.  4096
    constraints (log_n = 12) over 3000 wires.  The plan's counts are those of the untransposed rows (r1cs_cases.split_counts)."""
    src = RC.skewed_r1cs(n_constraints=3000, nb_wires=4096, nb_public=33, seed=1208)
    r1cs = RC.transposed(src)
    nw = r1cs["nb_wires"]
    assert r1cs["n_constraints"] == 4096 and nw == 3000
    td = S.synth_trapdoor(1209)
    got = ctx.setup_exponents(r1cs, td)
    st = ctx.setup_stats()
    print(f"setup_exponents at the split edges: {st}")
    assert (st["long_columns"], st["chunks"]) == RC.split_counts(src)
    assert st["entries"] == sum(len(r1cs[name][1]) for name in "ABC")
    RC.check_columns(r1cs, td, got, split_edge_wires(src, r1cs), seed=1210)
    S.check_z(td, 12, got["z"])


def split_edge_wires(src, r1cs):
    """name -> the columns test_setup_columns_at_the_split_edges recomputes in integers: the planted ones, the ends, an empty one, 32 random"""
    nw = r1cs["nb_wires"]
    wires = {0, 1, nw - 2, nw - 1} | {int(x) for x in np.random.default_rng(1211).integers(0, nw, 32)}
    out = {}
    for name in "ABC":
        lens = np.bincount(r1cs[name][1], minlength=nw)
        planted = src["long_at"][name]
        assert [int(lens[planted[n]]) for n in RC.LONG_LENS] == list(RC.LONG_LENS) and set(range(5)) <= set(lens.tolist())
        out[name] = wires | set(planted.values()) | {int(np.nonzero(lens == 0)[0][0])}
    return out


# ---------------------------------------------------------------------------------------------------- 3: whole key
WHOLE_KEY_LOG_N = 23


def test_setup_whole_key_at_the_benchmark_shape(ctx):
    B = load_binding()
    L_ = WHOLE_KEY_LOG_N
    N = 1 << L_
    ctx.trim()
    # 3 entries per live row, 97 % live rows: about 2.9 per row per matrix; one commitment over N / 32 wires
    r1cs = S.synth_r1cs(N - 100, nb_wires=N - 1000, nb_public=4097, seed=2222, per_row=3, n_coeffs=1 << 12, n_heavy=64, commitments=1, n_committed=N >> 5)
    td = S.synth_trapdoor(77, n_sigma=1)
    t0 = time.perf_counter()
    got = ctx.setup_exponents(r1cs, td)
    print(f"setup_exponents 2^{L_}: {time.perf_counter() - t0:.2f} s wall; {ctx.setup_stats()}")
    t0 = time.perf_counter()
    S.check_exponents(r1cs, td, got, seed=3)
    S.check_z(td, L_, got["z"])
    print(f"host reference of the exponents 2^{L_}: {time.perf_counter() - t0:.1f} s")
    e = S.dlog_exps(r1cs, td, got, L_)
    committed, cwire = r1cs["commitments"][0]
    nw = r1cs["nb_wires"]
    W = cref.gen_scalars(nw, 31, 1); W[0] = D.ONE
    a, b, _ = D.constraint_values(r1cs["n_constraints"], 1, 41)
    r, s = cref.gen_scalars(2, 51, 0)
    ch = cref.gen_scalars(1, 52, 0)[0]
    vals = np.ascontiguousarray(W[committed])
    want = D.expected_proof_exps(e, W, a, b, r, s)
    cm_exp = D._int(D.fr_dot(vals, got["k_gamma"][committed]))
    pool = B.Prover(0, 2)
    try:
        c0 = pool.ctx(0)
        t0 = time.perf_counter()
        pkh, peds, vk = c0.setup(r1cs, td)
        print(f"mi_groth16_setup 2^{L_}: {time.perf_counter() - t0:.2f} s wall; {c0.setup_stats()}; table plan {c0.pk_table_plan(pkh)}")
        try:
            cm = pool.commit(peds[0], vals)
            proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, r, s, [(peds[0], vals)], ch))
        finally:
            c0.pedersen_pk_free(peds[0])
            c0.pk_free(pkh)
    finally:
        pool.close()
    D.check_proof(proof, want)
    assert g1_pts(cm) == [P.g1_mul(P.G1_GEN, cm_exp)], "the commitment is not g^(sum v_i t_j / gamma)"
    assert g1_pts(proof["pok"]) == [P.g1_mul(P.G1_GEN, cm_exp * D._int(td["sigma"][0]) % P.R_MOD)], "the proof of knowledge is not g^(sigma * that)"
    # vk.G1.K: public wires, then the commitment wire
    rows = D.spot_rows(len(vk["k"]), vk["k"][:, :4], 5)
    wires = np.concatenate([np.arange(r1cs["nb_public"]), [cwire]])
    assert len(vk["k"]) == r1cs["nb_public"] + 1
    assert g1_pts(vk["k"][rows]) == [P.g1_mul(P.G1_GEN, x) for x in fr_vals(got["k_gamma"][wires[rows]])]


def test_setup_key_arrays_row_by_row(ctx):
    """64 spot rows of each point array of a setup-made key, as dlog_keys.spot_rows picks them.  The key consumes its compact arrays,
    so the rows are read through one-hot witnesses: a proof with W = e_j, a = b = 0, r = s = 0 has Ar = alpha1 + A_j g1,
    Bs = beta2 + B_j g2 and Krs = K_j g1 (j in K)."""
    log_n = 12
    N = 1 << log_n
    r1cs = S.synth_r1cs(N - 10, nb_wires=N + 50, nb_public=9, seed=12, per_row=4, n_coeffs=300, n_heavy=4, heavy_len=64, commitments=1, n_committed=40)
    td = S.synth_trapdoor(13, n_sigma=1)
    got = ctx.setup_exponents(r1cs, td)
    e = S.dlog_exps(r1cs, td, got, log_n)
    nw = r1cs["nb_wires"]
    pkh, peds, _ = ctx.setup(r1cs, td)
    try:
        zero = np.zeros((r1cs["n_constraints"], 4), np.uint64)
        z4 = np.zeros(4, np.uint64)
        for j in D.spot_rows(nw, got["a"], 1):
            W = np.zeros((nw, 4), np.uint64); W[j] = D.ONE
            proof, _ = ctx.prove(pkh, W, zero, zero, zero, z4, z4)
            D.check_proof(proof, D.expected_proof_exps(e, W, zero, zero, z4, z4))
        # the Pedersen bases row by row: a one-hot value vector
        committed = r1cs["commitments"][0][0]
        for i in D.spot_rows(len(committed), got["k_gamma"][committed], 2)[:16]:
            v = np.zeros((len(committed), 4), np.uint64); v[i] = D.ONE
            x = D._int(got["k_gamma"][committed[i]])
            assert g1_pts(ctx.pedersen_commit(peds[0], v)) == [P.g1_mul(P.G1_GEN, x)]
            assert g1_pts(ctx.pedersen_commit(peds[0], v, knowledge=True)) == [P.g1_mul(P.G1_GEN, x * D._int(td["sigma"][0]) % P.R_MOD)]
    finally:
        ctx.pedersen_pk_free(peds[0])
        ctx.pk_free(pkh)


# ---------------------------------------------------------------------------------------------------- 4: refusals
def _small():
    r1cs = S.synth_r1cs(500, nb_wires=700, nb_public=5, seed=4, per_row=3, n_coeffs=16, n_heavy=2, heavy_len=40, n_empty_cols=8, commitments=2, n_committed=6)
    return r1cs, S.synth_trapdoor(4, n_sigma=2)


def _mat(r1cs, name, rp=None, col=None, cf=None):
    m = list(r1cs[name])
    for i, x in enumerate((rp, col, cf)):
        if x is not None:
            m[i] = x
    return tuple(m)


def _refusals():
    r1cs, td = _small()
    tau_on_domain = fr_arr([pow(P.Domain(500).gen, 77, P.R_MOD)])[0]
    rp = r1cs["A"][0]
    bad_start = rp.copy(); bad_start[0] = 1
    decreasing = rp.copy(); decreasing[10] = decreasing[11] + 1
    col_hi = r1cs["B"][1].copy(); col_hi[17] = 700
    cf_hi = r1cs["C"][2].copy(); cf_hi[3] = 16
    com = r1cs["commitments"]
    zero = np.zeros(4, np.uint64)
    cases = {
        "A.row_ptr null": (dict(A=(None, r1cs["A"][1], r1cs["A"][2])), {}, "A.row_ptr"),
        "B.col null": (dict(B=(r1cs["B"][0], None, r1cs["B"][2])), {}, "B.col"),
        "coeffs null": (dict(coeffs=None, n_coeffs=16), {}, "coeffs"),
        "row_ptr[0] != 0": (dict(A=_mat(r1cs, "A", rp=bad_start)), {}, "A.row_ptr[0]"),
        "row_ptr decreases": (dict(A=_mat(r1cs, "A", rp=decreasing)), {}, "A.row_ptr"),
        "col >= nb_wires": (dict(B=_mat(r1cs, "B", col=col_hi)), {}, "B.col[17]"),
        "coeff >= n_coeffs": (dict(C=_mat(r1cs, "C", cf=cf_hi)), {}, "C.coeff[3]"),
        "log_n > 27": (dict(n_constraints=(1 << 27) + 1), {}, "n_constraints"),
        "nb_public 0": (dict(nb_public=0), {}, "nb_public"),
        "nb_public > nb_wires": (dict(nb_public=701), {}, "nb_public"),
        "committed wire public": (dict(commitments=[(np.array([2, 50], np.uint32), com[0][1]), com[1]]), {}, "committed[0][0]"),
        "commitment wire public": (dict(commitments=[(com[0][0], 1), com[1]]), {}, "commitment_wire[0]"),
        "wire listed twice": (dict(commitments=[com[0], (com[1][0], com[0][1])]), {}, "listed twice"),
        "too many commitments": (dict(n_commitments=17), {}, "n_commitments"),
        "delta 0": ({}, dict(delta=zero), "delta"),
        "gamma 0": ({}, dict(gamma=zero), "gamma"),
        "sigma 0": ({}, dict(sigma=[td["sigma"][0], zero]), "sigma[1]"),
        "tau on the domain": ({}, dict(tau=tau_on_domain), "tau"),
    }
    return r1cs, td, cases


@pytest.mark.parametrize("case", sorted(_refusals()[2]))
def test_setup_refusals(ctx, case):
    B = load_binding()
    r1cs, td, cases = _refusals()
    dr, dt, word = cases[case]
    before = ctx.mem_ledger()
    for call in (lambda x, y: ctx.setup_exponents(x, y), lambda x, y: ctx.setup(x, y)):
        with pytest.raises(B.MiError) as ei:
            call({**r1cs, **dr}, {**td, **dt})
        assert "rc=-1:" in str(ei.value) and word in str(ei.value), str(ei.value)
    assert ctx.mem_ledger() == before


def test_setup_refuses_null_arguments(ctx):
    import ctypes as C
    B = load_binding()
    r1cs, td = _small()
    d, keep = B._r1cs_desc(r1cs); t = B._trapdoor(td)
    e = B.SetupExponents(); h = C.c_void_p(); vk = B.VkOut(); ped = (C.c_void_p * 16)()
    lib = ctx.lib
    assert lib.mi_groth16_setup_exponents(ctx.h, None, C.byref(t), C.byref(e)) == -1
    assert lib.mi_groth16_setup_exponents(ctx.h, C.byref(d), None, C.byref(e)) == -1
    assert lib.mi_groth16_setup_exponents(ctx.h, C.byref(d), C.byref(t), None) == -1
    assert lib.mi_groth16_setup(ctx.h, C.byref(d), C.byref(t), None, ped, C.byref(vk)) == -1
    assert lib.mi_groth16_setup(ctx.h, C.byref(d), C.byref(t), C.byref(h), ped, None) == -1
    assert lib.mi_groth16_setup(ctx.h, C.byref(d), C.byref(t), C.byref(h), None, C.byref(vk)) == -1 and b"ped_out" in lib.mi_last_error(ctx.h)
    assert lib.mi_groth16_setup(ctx.h, C.byref(d), C.byref(t), C.byref(h), ped, C.byref(vk)) == -1 and b"k_cap" in lib.mi_last_error(ctx.h)   # vk.k null
    assert lib.mi_groth16_setup(None, C.byref(d), C.byref(t), C.byref(h), ped, C.byref(vk)) == -1
    assert not h.value


# ---------------------------------------------------------------------------------------------------- 5: an ordinary key
def test_setup_key_is_an_ordinary_key(ctx):
    """table plan and the key's ledger against mi_pk_load_dev of the same points (built from the same exponents by the existing
    batch scalar multiplication), with window tables forced so that both keys keep the same arrays; free and trim return everything"""
    log_n = 14
    N = 1 << log_n
    r1cs = S.synth_r1cs(N - 3, nb_wires=N + 100, nb_public=17, seed=14, per_row=4, n_coeffs=1000, n_heavy=8, heavy_len=200, commitments=1, n_committed=100)
    td = S.synth_trapdoor(15, n_sigma=1)
    ctx.trim()
    start = ctx.mem_ledger()
    got = ctx.setup_exponents(r1cs, td)
    e = S.dlog_exps(r1cs, td, got, log_n)
    key_part = lambda m: {k: v for k, v in m.items() if k.startswith("key_")}
    ctx_part = lambda m: {k: v for k, v in m.items() if k.startswith("ctx_")}
    W = cref.gen_scalars(r1cs["nb_wires"], 3, 1); a, b, _ = D.constraint_values(r1cs["n_constraints"], 1, 4); r, s = cref.gen_scalars(2, 5, 0)
    for knob in ((17, 17, 17), (0, 0, 0)):
        assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, *knob) == 0
        try:
            pkh, peds, _ = ctx.setup(r1cs, td)
            ref_pk, bufs = D.points_from_exps(e, ctx, device=True)
            ref = ctx.pk_load(ref_pk, device_points=True)
        finally:
            assert ctx.lib.mi_debug_set_prove_fixed_base(ctx.h, 0, 0, 0) == 0
        try:
            assert ctx.pk_table_plan(pkh) == ctx.pk_table_plan(ref)
            m_setup, m_ref = key_part(ctx.mem_ledger(pkh)), key_part(ctx.mem_ledger(ref))
            assert m_setup["key_tables"] == m_ref["key_tables"] and m_setup["key_indices"] == m_ref["key_indices"]
            if knob[0]:
                assert m_setup == m_ref      # with tables neither key keeps a plain copy of B or Z
            p1, _ = ctx.prove(pkh, W, a, b, None, r, s)
            p2, _ = ctx.prove(ref, W, a, b, None, r, s)
            assert np.array_equal(p1["raw"], p2["raw"])
        finally:
            ctx.pk_free(ref); ctx.pk_free(pkh); ctx.pedersen_pk_free(peds[0])
            for d in bufs:
                d.free()
        assert key_part(ctx.mem_ledger()) == key_part(start)
    # two Setups and frees in a row leave the context where it started once trimmed
    ctx.trim()
    base = ctx_part(ctx.mem_ledger())
    for _ in range(2):
        pkh, peds, _ = ctx.setup(r1cs, td)
        ctx.pk_free(pkh); ctx.pedersen_pk_free(peds[0])
    ctx.trim()
    assert ctx_part(ctx.mem_ledger()) == base
