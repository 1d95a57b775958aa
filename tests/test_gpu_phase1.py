"""GPU suite: phase 1 on the device (include/mi355x_groth16_phase1.h, csrc/phase1.hip, csrc/scale_powers.cuh): the scalar multiplication
out[i] = [c t^(k0 + i)] P[i] in every window width and by the bit-by-bit yardstick, contributions, their records, the verification of
claimed rows and the handover to phase 2.

The yardstick needs no new oracle.  Points with KNOWN discrete logs go in -- [e_i] g from mi_batch_scalar_mul_g1 / _g2, which is
oracle-checked elsewhere -- and the expected output is mi_batch_scalar_mul of the products computed in Python integers.  An affine point
has one encoding, so every comparison is array_equal."""
import ctypes as C
import hashlib
import numpy as np
import pytest
import pyref as P
import cref
import dlog_keys as D
import r1cs_cases as RC
import bytes_cases as BC
import test_gpu_phase2 as T2
import test_gpu_phase2_check as TK
from helpers import fr_arr, fr_vals, g1_arr, g1_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R = P.R_MOD
SEED = bytes(range(60, 92))
ROWS = ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2")
ROOT_256 = pow(P.FR_ROOT_2_28, 1 << (P.FR_TWO_ADICITY - 8), R)   # a primitive 256th root of unity: the scalars 1 and r - 1 occur inside a row
RAW, COMPRESSED = 0, 1
DEFAULT_WINDOW = 5   # the width measured fastest (profiles/phase1.txt)


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture()
def knobs(ctx):
    """sets knobs for one test and puts the defaults back"""
    yield ctx.set_knob
    ctx.set_knob("scale_powers_window", DEFAULT_WINDOW)
    ctx.set_knob("scale_powers_chunk", 0)


def fr1(v):
    return fr_arr([v % R])[0]


def points_of(ctx, exps, g2):
    return ctx.batch_scalar_mul(D.G2 if g2 else D.G1, TK.mont_rows([e % R for e in exps]), g2=g2)


def assert_rows_equal(got, want, what, rows=ROWS + ("beta_g2",)):
    for name in rows:
        assert np.array_equal(got[name], want[name]), f"{what}: {name}"


def known_srs(ctx, N, t, a, b):
    return TK.srs_points(ctx, TK.honest_exps(N, t, a, b))


# ---------------------------------------------------------------------------------------------------- 1: the kernel
SIZES = (1, 63, 64, 65, 200)
K0S = (0, 1, (1 << 27) - 100)


def input_exps(n):
    """the discrete logs of the points that go in: random, some 0 (the point at infinity), three copies of one point"""
    rng = P.SplitMix64(900 + n)
    e = [rng.fr() for _ in range(n)]
    if n >= 8:
        e[2] = e[7] = 0
        e[4] = e[5] = e[3]
    if n >= 64:
        e[63] = 0
        e[n - 1] = e[0]
    return e


def scalar_cases():
    rng = P.SplitMix64(77)
    t, c1, c2, c3 = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    # (name, t, c): c = 1 where the point of the case is the scalar t^k itself
    return [("random", t, c1), ("one", 1, c2), ("minus one", R - 1, c3), ("two", 2, 1), ("root of unity", ROOT_256, 1)]


@pytest.fixture(scope="module")
def scale_inputs(ctx):
    """per (g2, n): the exponents, the points, and per (case, k0) the expected points -- computed once, shared by every window width"""
    out = {}
    assert pow(ROOT_256, 128, R) == R - 1
    for g2 in (False, True):
        for n in SIZES:
            e = input_exps(n)
            pts = points_of(ctx, e, g2)
            assert (not pts[2].any()) if n >= 8 else True   # a zero exponent is (0, 0)
            want = {}
            for name, t, c in scalar_cases():
                for k0 in K0S:
                    s = c * pow(t, k0, R) % R
                    prod = []
                    for i in range(n):
                        prod.append(e[i] * s % R)
                        s = s * t % R
                    want[name, k0] = points_of(ctx, prod, g2)
            out[g2, n] = (pts, want)
    return out


@pytest.mark.parametrize("w", [0, 2, 3, 4, 5])
@pytest.mark.parametrize("g2", [False, True], ids=["G1", "G2"])
def test_scale_powers_equals_known_exponents(ctx, knobs, scale_inputs, g2, w):
    knobs("scale_powers_window", w)
    knobs("scale_powers_chunk", 64)   # 65 and 200 cross chunk ends, with a short last chunk
    for n in SIZES:
        pts, want = scale_inputs[g2, n]
        for name, t, c in scalar_cases():
            for k0 in K0S:
                got = ctx.debug_scale_powers(pts, fr1(t), fr1(c), k0, g2=g2)
                assert np.array_equal(got, want[name, k0]), f"w = {w}, n = {n}, t: {name}, k0 = {k0}"
        st = ctx.phase1_stats()
        assert st["window"] == w and st["chunk"] == 64


def test_scale_powers_refusals(ctx):
    B = load_binding()
    pts = points_of(ctx, [5, 6], False)
    not_below_r = np.frombuffer(R.to_bytes(32, "little"), np.uint64)
    with pytest.raises(B.MiError):
        ctx.debug_scale_powers(pts, not_below_r, fr1(1))
    with pytest.raises(B.MiError):
        ctx.debug_scale_powers(pts, fr1(3), fr1(1), k0=(1 << 64) - 1)
    for name, v in (("scale_powers_window", 1), ("scale_powers_window", 6), ("scale_powers_chunk", 63), ("scale_powers_chunk", (1 << 24) + 1)):
        with pytest.raises(B.MiError):
            ctx.set_knob(name, v)
    assert ctx.lib.mi_debug_scale_powers_dev(ctx.h, C.c_int32(0), None, C.c_size_t(2), None, None, C.c_uint64(0), None) == -1
    assert ctx.debug_scale_powers(pts[:0], fr1(3), fr1(1)).shape == (0, 8)


# ---------------------------------------------------------------------------------------------------- 2: contributions
@pytest.mark.parametrize("log_n", [1, 2, 5, 6])   # 2 N = 64 is exactly one wave of tau_g1, 2 N = 128 two
def test_contribution_equals_the_known_exponent_srs(ctx, log_n):
    N = 1 << log_n
    t1, a1, b1, _ = T2.secrets(7000 + log_n)
    t2, a2, b2, _ = T2.secrets(7100 + log_n)
    st = ctx.phase1_init(log_n)
    other = None
    try:
        first = ctx.phase1_export(st)
        assert_rows_equal(first, known_srs(ctx, N, 1, 1, 1), "init: every row the generator")
        ctx.phase1_contribute(st, fr1(t1), fr1(a1), fr1(b1))
        want1 = known_srs(ctx, N, t1, a1, b1)
        assert_rows_equal(ctx.phase1_export(st), want1, "one contribution")
        s = ctx.phase1_stats()
        print(f"phase1 contribute log_n = {log_n}: {s}")
        assert s["window"] == DEFAULT_WINDOW and s["total_ms"] > 0 and s["peak_bytes"] > 0
        ctx.phase1_contribute(st, fr1(t2), fr1(a2), fr1(b2))
        want2 = known_srs(ctx, N, t1 * t2 % R, a1 * a2 % R, b1 * b2 % R)
        assert_rows_equal(ctx.phase1_export(st), want2, "two contributions: the products")
        assert ctx.phase1_check(st, SEED) == 0 and ctx.phase1_check(st, None) == 0
        other = ctx.phase1_from_srs(want1, N)
        ctx.phase1_contribute(other, fr1(t2), fr1(a2), fr1(b2))
        assert_rows_equal(ctx.phase1_export(other), want2, "an SRS taken in, then a contribution")
        info = ctx.phase1_info(other)
        assert info["log_n"] == log_n and info["n_records"] == 0 and info["chain"] == bytes(32)
        assert np.array_equal(info["tau1"], want2["tau_g1"][1]) and np.array_equal(info["alpha1"], want2["alpha_tau_g1"][0]) and np.array_equal(info["beta1"], want2["beta_tau_g1"][0])
    finally:
        ctx.phase1_free(st)
        if other is not None:
            ctx.phase1_free(other)


def test_contribution_by_the_yardstick_and_every_width_gives_the_same_rows(ctx, knobs):
    N = 32
    t, a, b, _ = T2.secrets(7300)
    want = known_srs(ctx, N, t, a, b)
    for w in (0, 2, 3, 4):
        knobs("scale_powers_window", w)
        st = ctx.phase1_init(5)
        try:
            ctx.phase1_contribute(st, fr1(t), fr1(a), fr1(b))
            assert_rows_equal(ctx.phase1_export(st), want, f"w = {w}")
            assert ctx.phase1_stats()["window"] == w
        finally:
            ctx.phase1_free(st)


# ---------------------------------------------------------------------------------------------------- 3: past the default chunk
def test_row_of_twice_the_chunk(ctx, knobs):
    """2 N = twice the chunk: tau_g1 takes two full chunks, tau_g2 exactly one.  The default chunk (2^18) would make this a row of 2^19
    points; the knob lowers it to 2^16, and the test reads the chunk the driver says it ran with"""
    knobs("scale_powers_chunk", 1 << 16)
    ctx.debug_scale_powers(points_of(ctx, [1], False), fr1(1), fr1(1))
    chunk = ctx.phase1_stats()["chunk"]
    assert chunk == 1 << 16
    log_n = chunk.bit_length() - 1
    N = 1 << log_n
    t, a, b, _ = T2.secrets(7400)
    pw = [1]
    for _ in range(2 * N - 1):
        pw.append(pw[-1] * t % R)
    st = ctx.phase1_init(log_n)
    try:
        ctx.phase1_contribute(st, fr1(t), fr1(a), fr1(b))
        stats = ctx.phase1_stats()
        print(f"phase1 contribute log_n = {log_n}: {stats}")
        assert stats["chunk"] == chunk
        got = ctx.phase1_export(st)
        assert np.array_equal(got["tau_g1"], ctx.batch_scalar_mul(D.G1, TK.mont_rows(pw)))
        assert np.array_equal(got["tau_g2"], ctx.batch_scalar_mul(D.G2, TK.mont_rows(pw[:N]), g2=True))
    finally:
        ctx.phase1_free(st)


# ---------------------------------------------------------------------------------------------------- 4, 5: proved contributions, adoption
def record_hash(prev, index, before, after, commit):
    return hashlib.sha256(b"mi355x-phase1-record" + prev + index.to_bytes(8, "little") + b"".join(P.g1_compress(p) for p in before + after + commit)).digest()


def challenge(h):
    return int.from_bytes(hashlib.sha256(b"mi355x-phase1-challenge" + h).digest()[:16], "little")


def restated_record(prev, index, e_before, d, k):
    """the record of a step in Python: pyref's points, hashlib's hashes -> (64,) uint64, the hash"""
    before = [P.g1_mul(P.G1_GEN, e) for e in e_before]
    after = [P.g1_mul(P.G1_GEN, e * x % R) for e, x in zip(e_before, d)]
    commit = [P.g1_mul(P.G1_GEN, e * x % R) for e, x in zip(e_before, k)]
    h = record_hash(prev, index, before, after, commit)
    c = challenge(h)
    out = np.zeros(64, np.uint64)
    out[:24] = g1_arr(after).reshape(-1)
    out[24:48] = g1_arr(commit).reshape(-1)
    out[48:60] = fr_arr([(kk + c * dd) % R for kk, dd in zip(k, d)]).reshape(-1)
    out[60:] = np.frombuffer(h, np.uint64)
    return out, h


LOG_N_ADOPT = 3
ID = hashlib.sha256(b"a phase-1 transcript").digest()


@pytest.fixture(scope="module")
def contributed(ctx):
    """A: init, a transcript id, two proved contributions with given nonces -> (the factors, A's export, the records, A's info)"""
    rng = P.SplitMix64(7500)
    steps = [([rng.fr() for _ in range(3)], [rng.fr() for _ in range(3)]) for _ in range(2)]   # (t, a, b), nonces
    a = ctx.phase1_init(LOG_N_ADOPT)
    try:
        ctx.phase1_set_transcript_id(a, ID)
        recs = np.stack([ctx.phase1_contribute_proved(a, *(fr1(v) for v in d), fr_arr(k)) for d, k in steps])
        return steps, ctx.phase1_export(a), recs, ctx.phase1_info(a)
    finally:
        ctx.phase1_free(a)


def fresh_b(ctx):
    b = ctx.phase1_init(LOG_N_ADOPT)
    ctx.phase1_set_transcript_id(b, ID)
    return b


def test_records_equal_their_restatement_and_verify_on_the_host(ctx, contributed):
    B = load_binding()
    steps, rows, recs, info = contributed
    e, prev = [1, 1, 1], ID
    for i, (d, k) in enumerate(steps):
        want, prev = restated_record(prev, i, e, d, k)
        assert np.array_equal(recs[i], want), f"record {i}"
        e = [x * y % R for x, y in zip(e, d)]
    g = np.repeat(g1_arr([P.G1_GEN]), 3, axis=0)
    assert B.phase1_records_verify(g, ID, 0, recs) == 2
    assert B.phase1_records_verify(g, bytes(32), 0, recs) == 0 and B.phase1_records_verify(g, ID, 1, recs) == 0
    assert info["n_records"] == 2 and info["chain"] == recs[1, 60:].tobytes()
    N = 1 << LOG_N_ADOPT
    assert_rows_equal(rows, known_srs(ctx, N, *(steps[0][0][x] * steps[1][0][x] % R for x in range(3))), "A after two proved contributions")


def test_verify_adopt_takes_honest_rows_and_the_chain_goes_on(ctx, contributed):
    B = load_binding()
    steps, rows, recs, info = contributed
    b = fresh_b(ctx)
    try:
        assert ctx.phase1_verify_adopt(b, rows, recs, SEED) == (0, 2)
        assert_rows_equal(ctx.phase1_export(b), rows, "B after adoption")
        got = ctx.phase1_info(b)
        assert got["n_records"] == 2 and got["chain"] == info["chain"] and all(np.array_equal(got[k], info[k]) for k in ("tau1", "alpha1", "beta1"))
        rng = P.SplitMix64(7600)
        d, k = [rng.fr() for _ in range(3)], [rng.fr() for _ in range(3)]
        rec3 = ctx.phase1_contribute_proved(b, *(fr1(v) for v in d), fr_arr(k))
        e = [steps[0][0][x] * steps[1][0][x] % R for x in range(3)]
        assert np.array_equal(rec3, restated_record(info["chain"], 2, e, d, k)[0])
        start = np.stack([info["tau1"], info["alpha1"], info["beta1"]])
        assert B.phase1_records_verify(start, info["chain"], 2, rec3.reshape(1, -1)) == 1
        g = np.repeat(g1_arr([P.G1_GEN]), 3, axis=0)
        assert B.phase1_records_verify(g, ID, 0, np.vstack([recs, rec3.reshape(1, -1)])) == 3
        # a contribution drawn from the operating system's nonces verifies too
        rec4 = ctx.phase1_contribute_proved(b, *(fr1(v) for v in d), None)
        assert B.phase1_records_verify(g, ID, 0, np.vstack([recs, rec3.reshape(1, -1), rec4.reshape(1, -1)])) == 4
    finally:
        ctx.phase1_free(b)


def _tampered(ctx, contributed, what):
    """-> (claim, records, expected mask or None for MI_EINVAL, expected first_bad_record, text the error must hold)"""
    B = load_binding()
    steps, rows, recs, _ = contributed
    claim = {k: v.copy() for k, v in rows.items()}
    recs = recs.copy()
    other_g1 = points_of(ctx, [123456789], False)[0]
    other_g2 = points_of(ctx, [123456789], True)[0]
    N = 1 << LOG_N_ADOPT
    t, a, b = (steps[0][0][x] * steps[1][0][x] % R for x in range(3))
    if what in ("tau_g1[3]", "alpha_tau_g1[3]", "beta_tau_g1[3]", "tau_g2[3]"):
        # the expected mask is computed in the exponent (test_gpu_phase2_check.model_mask): tau_g1[3] lies below N, so it enters the
        # tau_g2 relation as well
        row = what[:-3]
        exps = TK.honest_exps(N, t, a, b)
        exps[row][3] = 123456789
        claim[row][3] = other_g2 if row == "tau_g2" else other_g1
        want = TK.model_mask(B, exps, N, SEED)
        bit = {"tau_g1": B.SRS_BAD_TAU_G1, "alpha_tau_g1": B.SRS_BAD_ALPHA_G1, "beta_tau_g1": B.SRS_BAD_BETA_G1, "tau_g2": B.SRS_BAD_TAU_G2}[row]
        assert want & bit and want == (bit | (B.SRS_BAD_TAU_G2 if row == "tau_g1" else 0))
        return claim, recs, want, 2, None
    if what == "beta_g2":
        claim["beta_g2"] = points_of(ctx, [b + 1], True)[0]
        return claim, recs, B.SRS_BAD_BETA_G2, 2, None
    if what == "another tau":
        return known_srs(ctx, N, t + 1, a, b), recs, B.PHASE1_BAD_LINK, 2, None
    if what == "response":
        recs[1, 52:56] = fr_arr([(fr_vals(recs[1, 52:56].reshape(1, 4))[0] + 1) % R])[0]
        return claim, recs, B.PHASE1_BAD_RECORD, 1, None
    if what == "off the curve":
        claim["tau_g2"][5, 0] ^= np.uint64(1)
        return claim, recs, None, None, "srs.tau_g2[5]"
    if what == "at infinity":
        claim["alpha_tau_g1"][6] = 0
        return claim, recs, None, None, "srs.alpha_tau_g1[6]"
    raise AssertionError(what)


@pytest.mark.parametrize("what", ["tau_g1[3]", "alpha_tau_g1[3]", "beta_tau_g1[3]", "tau_g2[3]", "beta_g2", "another tau", "response", "off the curve", "at infinity"])
def test_verify_adopt_rejections_leave_the_state_as_it_was(ctx, contributed, what):
    B = load_binding()
    claim, recs, mask, first_bad, text = _tampered(ctx, contributed, what)
    b = fresh_b(ctx)
    try:
        before_rows, before_info = ctx.phase1_export(b), ctx.phase1_info(b)
        if mask is None:
            with pytest.raises(B.MiError, match="rc=-1") as ei:
                ctx.phase1_verify_adopt(b, claim, recs, SEED)
            assert text in str(ei.value)
        else:
            assert ctx.phase1_verify_adopt(b, claim, recs, SEED) == (mask, first_bad), what
        assert_rows_equal(ctx.phase1_export(b), before_rows, "B after a rejection")
        after = ctx.phase1_info(b)
        assert after["n_records"] == 0 and after["chain"] == ID == before_info["chain"] and np.array_equal(after["tau1"], before_info["tau1"])
        # and the honest claim is still taken afterwards
        assert ctx.phase1_verify_adopt(b, contributed[1], contributed[2], SEED) == (0, 2)
    finally:
        ctx.phase1_free(b)


# ---------------------------------------------------------------------------------------------------- 6: end to end
def test_phase1_to_phase2_to_a_proof_that_verifies(ctx):
    """init(7), two proved contributions, the rows check; phase 2 from the state's device arrays and from its export both equal Setup for
    the products of the factors; one proof through the sealed key verifies from its bytes"""
    B = load_binding()
    ncom, n, nab, nb_public = 2, 100, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 51, long_lens=(16, 17), commitments=ncom, n_committed=7)
    r1cs["commitments"] = sorted(r1cs["commitments"], key=lambda c: c[1])   # by ascending commitment wire, as the bytes path reads them
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 52)
    rng = P.SplitMix64(7700)
    d1, d2 = [rng.fr() for _ in range(3)], [rng.fr() for _ in range(3)]
    sigma = [rng.fr() for _ in range(ncom)]
    sg = [fr1(s) for s in sigma]
    td = T2.trapdoor(*(x * y % R for x, y in zip(d1, d2)), 1, sigma)
    rr, ss = cref.gen_scalars(2, 71, 0)
    p1 = ctx.phase1_init(7)
    states, keys = [], []
    pool = B.Prover(0, 1)
    try:
        recs = np.stack([ctx.phase1_contribute_proved(p1, *(fr1(v) for v in d), None) for d in (d1, d2)])
        g = np.repeat(g1_arr([P.G1_GEN]), 3, axis=0)
        assert B.phase1_records_verify(g, bytes(32), 0, recs) == 2
        assert ctx.phase1_check(p1, SEED) == 0
        states.append(ctx.phase2_init_from_phase1(r1cs, p1, sg))
        states.append(ctx.phase2_init(r1cs, ctx.phase1_export(p1), sg))
        for enc in (RAW, COMPRESSED):   # Setup's streams once per encoding, both routes against them
            want_pk, want_vk = ctx.setup_to_streams(r1cs, td, enc, build=False)[:2]
            for route, st in zip(("from the device rows", "from the export"), states):
                got_pk, got_vk = ctx.phase2_to_streams(st, enc)
                assert got_vk == want_vk and got_pk == want_pk, f"{route}, encoding {enc}"
        _, vk_stream = ctx.phase2_to_streams(states[0], COMPRESSED)
        keys.append(ctx.phase2_seal(states[0], nb_public + ncom, ncom))
        pkh, peds, _ = keys[0]
        pub = fr_vals(W[1:nb_public])
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
        cms = np.stack([pool.commit(peds[k], vals[k]).reshape(8) for k in range(ncom)])
        values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
        for (_, cw), v in zip(r1cs["commitments"], values):
            W[cw] = fr_arr([v])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, rr, ss, [(peds[k], vals[k]) for k in range(ncom)], fr_arr([fold])[0]))
        blob = B.proof_write(proof["raw"], commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8))
        vkh = ctx.vk_load_stream(vk_stream)
        try:
            assert vkh.verify_bytes(blob, np.ascontiguousarray(W[1:nb_public])) == B.VERIFY_OK
            W[1, 0] ^= np.uint64(1)
            assert vkh.verify_bytes(blob, np.ascontiguousarray(W[1:nb_public])) != B.VERIFY_OK
        finally:
            vkh.free()
    finally:
        pool.close()
        for pkh, peds, _ in keys:
            T2.free_key(ctx, pkh, peds)
        for st in states:
            ctx.phase2_free(st)
        ctx.phase1_free(p1)


# ---------------------------------------------------------------------------------------------------- 7: refusals
def test_phase1_refusals(ctx, contributed):
    B = load_binding()
    lib = ctx.lib
    for log_n in (0, 28):
        with pytest.raises(B.MiError, match="log_n"):
            ctx.phase1_init(log_n)
    h = C.c_void_p()
    assert lib.mi_phase1_init(ctx.h, C.c_uint32(3), None) == -1 and lib.mi_phase1_init(None, C.c_uint32(3), C.byref(h)) == -1
    st = ctx.phase1_init(2)
    try:
        before = ctx.phase1_export(st)
        one = fr1(1)
        for args, word in (((fr1(0), one, one), "tau is 0"), ((one, fr1(0), one), "alpha is 0"), ((one, one, fr1(0)), "beta is 0"), ((None, one, one), "tau is null"),
                           ((one, one, np.frombuffer(R.to_bytes(32, "little"), np.uint64)), "beta is not below r")):
            with pytest.raises(B.MiError, match=word):
                ctx.phase1_contribute(st, *args)
            with pytest.raises(B.MiError, match=word):
                ctx.phase1_contribute_proved(st, *args, fr_arr([3, 4, 5]))
        with pytest.raises(B.MiError, match="nonce"):
            ctx.phase1_contribute_proved(st, one, one, one, fr_arr([3, 0, 5]))
        assert lib.mi_phase1_contribute_proved(ctx.h, st, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), None, None) == -1
        assert lib.mi_phase1_contribute(ctx.h, None, None, None, None) == -1 and lib.mi_phase1_free(ctx.h, None) == -1
        assert lib.mi_phase1_check(ctx.h, st, None, None) == -1 and lib.mi_phase1_check(ctx.h, None, None, C.byref(C.c_uint32())) == -1
        assert lib.mi_phase1_get_stats(ctx.h, None) == -1 and lib.mi_phase1_get_info(ctx.h, st, None) == -1
        assert lib.mi_phase1_export(ctx.h, st, None, None, None, None, None, *(C.c_uint64(0),) * 4, None) == -1
        assert lib.mi_phase1_verify_adopt(ctx.h, st, None, None, C.c_size_t(1), None, C.byref(C.c_uint32()), None) == -1
        with pytest.raises(B.MiError, match="m is 0"):
            ctx.phase1_verify_adopt(st, before, np.zeros((0, B.PHASE1_RECORD_WORDS), np.uint64), SEED)
        with pytest.raises(B.MiError, match="n_tau_g2"):   # a claim for a smaller domain is a short row
            ctx.phase1_verify_adopt(st, {**before, "tau_g2": before["tau_g2"][:3]}, contributed[2], SEED)
        for i, cap in enumerate(((7, 4, 4, 4), (8, 3, 4, 4), (8, 4, 0, 4), (8, 4, 4, 3))):
            with pytest.raises(B.MiError, match=ROWS[i]):
                ctx.phase1_export(st, caps=cap)
        assert_rows_equal(ctx.phase1_export(st), before, "after the refusals")
        # the transcript id: before the first record only
        ctx.phase1_set_transcript_id(st, ID)
        ctx.phase1_contribute_proved(st, fr1(3), fr1(5), fr1(7), fr_arr([3, 4, 5]))
        with pytest.raises(B.MiError, match="before the first record"):
            ctx.phase1_set_transcript_id(st, bytes(32))
        assert lib.mi_phase1_set_transcript_id(ctx.h, st, None) == -1
        # a circuit larger than the state: N = 4 here, 5 constraints need 8
        big = RC.skewed_r1cs(5, 12, 3, 9, long_lens=())
        with pytest.raises(B.MiError, match="the circuit needs"):
            ctx.phase2_init_from_phase1(big, st)
        small = RC.skewed_r1cs(4, 12, 3, 9, long_lens=())
        p2 = ctx.phase2_init_from_phase1(small, st)
        ctx.phase2_free(p2)
        assert lib.mi_phase2_init_from_phase1(ctx.h, None, st, None, C.c_uint32(0), C.byref(h)) == -1
        d, keep = B._r1cs_desc(small)
        assert lib.mi_phase2_init_from_phase1(ctx.h, C.byref(d), None, None, C.c_uint32(0), C.byref(h)) == -1 and not h.value
    finally:
        ctx.phase1_free(st)
    srs = known_srs(ctx, 4, 3, 5, 7)
    with pytest.raises(B.MiError, match="n_domain"):
        ctx.phase1_from_srs(srs, 3)
    with pytest.raises(B.MiError, match="n_tau_g1"):
        ctx.phase1_from_srs(srs, 8)
    bad = {k: v.copy() for k, v in srs.items()}
    bad["beta_tau_g1"][2, 5] ^= np.uint64(4)
    with pytest.raises(B.MiError, match=r"srs\.beta_tau_g1\[2\]"):
        ctx.phase1_from_srs(bad, 4)
    with pytest.raises(B.MiError, match="unknown flag"):
        ctx.phase1_from_srs(srs, 4, flags=8)
