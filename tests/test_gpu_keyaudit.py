"""GPU: a key audited against its circuit and an SRS (include/mi355x_groth16_keyaudit.h, csrc/keyaudit.hip).

Keys come from mi_groth16_setup_to_streams with a known trapdoor whose gamma and delta are NOT 1; the SRS is built from the same
(tau, alpha, beta) through mi_batch_scalar_mul_g1 / _g2; the seeds are fixed.  The verdicts are exact: a mask is compared bit for bit.

1  an honest key audits to 0: from streams (both encodings), from arrays, from a phase-2 state before and after two contributions with
   sigma factors; SRS as host rows and as a phase-1 state
2  N = 8, one commitment: mi_debug_key_audit_sums against tests/keyaudit_ref.py's points, relation by relation
3  every tamper gives exactly its mask
4  refusals, the memory ledger unmoved
"""
import numpy as np
import pytest
import pyref as P
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
import verify_cases as V
import keyaudit_ref as KR
from helpers import fr_arr, g1_arr, g2_arr, g1_pts, g2_pts
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R = P.R_MOD
RAW, COMPRESSED = 0, 1
SEED = bytes(range(1, 33))
SEED2 = bytes(range(101, 133))


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def domain_size(nc):
    return 1 << max(nc - 1, 0).bit_length()


def make_srs(ctx, n, tau, alpha, beta):
    pw = [1]
    for _ in range(2 * n - 1):
        pw.append(pw[-1] * tau % R)
    return {"tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr(pw)),
            "alpha_tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr([alpha * p % R for p in pw[:n]])),
            "beta_tau_g1": ctx.batch_scalar_mul(D.G1, fr_arr([beta * p % R for p in pw[:n]])),
            "tau_g2": ctx.batch_scalar_mul(D.G2, fr_arr(pw[:n]), g2=True),
            "beta_g2": ctx.batch_scalar_mul(D.G2, fr_arr([beta]), g2=True)[0]}


def secrets(seed, n_sigma):
    rng = P.SplitMix64(seed)
    s = {n: rng.fr() for n in ("tau", "alpha", "beta", "gamma", "delta")}
    s["sigma"] = [rng.fr() for _ in range(n_sigma)]
    assert s["gamma"] != 1 and s["delta"] != 1
    return s


def trapdoor(s):
    td = {n: fr_arr([s[n]])[0] for n in ("tau", "alpha", "beta", "gamma", "delta")}
    td["sigma"] = [fr_arr([x])[0] for x in s["sigma"]]
    return td


class Case:
    """a circuit, its trapdoor, its SRS on the host, its key as two streams per encoding and as numpy arrays"""

    def __init__(self, ctx, r1cs, seed):
        self.r1cs, self.nc = r1cs, len(r1cs["commitments"])
        self.s = secrets(seed, self.nc)
        self.N = domain_size(r1cs["n_constraints"])
        self.srs = make_srs(ctx, self.N, self.s["tau"], self.s["alpha"], self.s["beta"])
        self.streams = {}
        for enc in (RAW, COMPRESSED):
            pk, vk, _, _, self.vk = ctx.setup_to_streams(r1cs, trapdoor(self.s), enc, build=False)
            self.streams[enc] = (pk, vk)
        self.vk_ped = ctx.pedersen_vk_make(np.array(trapdoor(self.s)["sigma"], np.uint64).reshape(-1, 4)) if self.nc else None
        self.arrays = decode(ctx, self.streams[COMPRESSED][0])


def decode(ctx, blob):
    """a compressed proving key's stream -> numpy: the five arrays, the Pedersen pairs, the small points, the masks"""
    B = load_binding()
    info, enc = B.pk_stream_inspect(blob)
    assert enc == COMPRESSED
    raw = np.frombuffer(blob, np.uint8)

    def points(off, n, g2=False):
        w = 16 if g2 else 8
        if not n:
            return np.zeros((0, w), np.uint64)
        size = 64 if g2 else 32
        src = ctx.to_dev(raw[off:off + size * n].copy()); dst = ctx.alloc(max(8 * w * n, 32))
        try:
            rc, bad = ctx.decompress_dev(src.ptr, n, dst.ptr, g2=g2)
            assert rc == 0 and bad == B.NO_BAD_INDEX
            return dst.download((n, w))
        finally:
            src.free(); dst.free()

    def mask(off):
        bits = np.unpackbits(raw[off:off + (info.nb_wires + 7) // 8])
        return bits[:info.nb_wires].astype(np.uint8)

    small1, small2 = points(info.off_alpha1, 3), points(info.off_beta2, 2, True)
    return {"log_n": info.log_n, "nb_wires": info.nb_wires, "g1_a": points(info.off_g1_a, info.n_g1_a), "g1_b": points(info.off_g1_b, info.n_g1_b),
            "g1_k": points(info.off_g1_k, info.n_g1_k), "g1_z": points(info.off_g1_z, info.n_g1_z), "g2_b": points(info.off_g2_b, info.n_g2_b, True),
            "alpha1": small1[0], "beta1": small1[1], "delta1": small1[2], "beta2": small2[0], "delta2": small2[1],
            "infinity_a": mask(info.off_infinity_a), "infinity_b": mask(info.off_infinity_b),
            "ped": [(points(info.off_basis[k], info.n_basis[k]), points(info.off_basis_exp_sigma[k], info.n_basis[k])) for k in range(info.n_commitment_keys)]}


class ArrayClaim:
    """mi_key_claim_from_arrays over numpy arrays: uploads, makes the claim, frees everything on exit.  counts: name -> a count that
    overrides the array's own"""

    def __init__(self, ctx, arrays, vk, vk_ped, counts=None, n_ped=None):
        self.ctx, self.bufs, self.h = ctx, [], None
        counts = counts or {}
        pk = {k: arrays[k] for k in ("log_n", "nb_wires", "alpha1", "beta1", "delta1", "beta2", "delta2", "infinity_a", "infinity_b")}
        pk["nb_wires"] = counts.get("nb_wires", pk["nb_wires"])
        for name in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b"):
            pk[name] = (self._up(arrays[name]), counts.get(name, len(arrays[name])))
        ped = [(self._up(b), self._up(e), counts.get(f"basis{k}", len(b))) for k, (b, e) in enumerate(arrays["ped"])]
        ped = ped if n_ped is None else ped[:n_ped]
        try:
            self.h = ctx.key_claim_from_arrays(pk, ped, vk, vk_ped, n_vk=counts.get("vk_k"))
        except Exception:
            self.close()
            raise

    def _up(self, a):
        b = self.ctx.to_dev(a if len(a) else np.zeros(8, np.uint64))
        self.bufs.append(b)
        return b.ptr

    def close(self):
        if self.h is not None:
            self.ctx.key_claim_free(self.h)
        for b in self.bufs:
            b.free()
        self.h, self.bufs = None, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def small_r1cs(nc, n_commitments, seed):
    return S.synth_r1cs(nc, nb_wires=max(48, nc + 40), nb_public=5, seed=seed, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=min(40, nc), n_empty_cols=6,
                        commitments=n_commitments, n_committed=3)


_cases = {}


def case_of(ctx, name):
    if name not in _cases:
        if name == "empty wires":
            # wire 9 (private) and wire 1 (public) are in no constraint: K holds an infinity slot with both mask bytes set, vk.K one too
            ent = {"A": [(0, 0, 1), (1, 2, 2), (2, 5, 1), (3, 6, 3), (4, 7, 1), (5, 8, 2)], "B": [(0, 3, 1), (1, 4, 1), (2, 0, 2), (4, 6, 1), (5, 10, 3)],
                   "C": [(0, 5, 1), (1, 6, 1), (2, 7, 1), (3, 8, 1), (4, 10, 1), (5, 11, 1)]}
            r1cs = {"n_constraints": 6, "nb_wires": 12, "nb_public": 3, "coeffs": fr_arr([0, 1, 5, R - 2]), "commitments": [(np.array([6, 7], np.uint32), 8)]}
            for m in "ABC":
                es = sorted(ent[m])
                rp = np.zeros(7, np.uint64)
                for row, _, _ in es:
                    rp[row + 1] += 1
                r1cs[m] = (np.cumsum(rp).astype(np.uint64), np.array([c for _, c, _ in es], np.uint32), np.array([k for _, _, k in es], np.uint32))
            _cases[name] = Case(ctx, r1cs, 900)
        elif name == "synth 2^12":
            r1cs = S.synth_r1cs(4000, nb_wires=4400, nb_public=9, seed=12, per_row=4, n_coeffs=256, n_heavy=3, heavy_len=1600, n_empty_cols=16,
                                commitments=1, n_committed=5)
            _cases[name] = Case(ctx, r1cs, 901)
        elif name == "long rows":
            # rows of 513 and 5000 entries in every matrix: the piece and combine passes of the product by rows
            r1cs = RC.skewed_r1cs(1500, 900, 7, seed=3, long_lens=(17, 512, 513, 5000), n_coeffs=128, commitments=2, n_committed=4)
            _cases[name] = Case(ctx, r1cs, 902)
        else:
            nc, n_com = name
            _cases[name] = Case(ctx, small_r1cs(nc, n_com, 10 * nc + n_com), 1000 + 10 * nc + n_com)
    return _cases[name]


SMALL_CASES = [(5, 0), (5, 1), (5, 2), (100, 0), (100, 1), (100, 2)]


def audit_streams(ctx, c, enc=COMPRESSED, seed=SEED, streams=None, srs=None, **kw):
    pk, vk = streams or c.streams[enc]
    h = ctx.key_claim_from_streams(pk, vk)
    try:
        return ctx.key_audit(c.r1cs, h, srs=srs or c.srs, seed=seed, **kw)
    finally:
        ctx.key_claim_free(h)


def audit_arrays(ctx, c, arrays=None, vk=None, seed=SEED, srs=None):
    with ArrayClaim(ctx, arrays or c.arrays, vk or c.vk, c.vk_ped) as cl:
        return ctx.key_audit(c.r1cs, cl.h, srs=srs or c.srs, seed=seed)


# ---------------------------------------------------------------------------------------------------- 1: an honest key
@pytest.mark.parametrize("name", SMALL_CASES + ["empty wires", "synth 2^12", "long rows"], ids=str)
def test_an_honest_key_audits_to_zero_from_streams_and_arrays(ctx, name):
    c = case_of(ctx, name)
    for enc in (RAW, COMPRESSED):
        assert audit_streams(ctx, c, enc) == 0, f"encoding {enc}"
    assert audit_streams(ctx, c, seed=SEED2) == 0
    st = ctx.key_audit_stats()
    print(f"key audit {name}: {st}")
    assert st["relations"] == 5 + c.nc and st["peak_bytes"] > 0 and st["total_ms"] > 0
    assert audit_arrays(ctx, c) == 0
    if name == "empty wires":
        a = c.arrays
        assert a["infinity_a"][9] and a["infinity_b"][9] and a["infinity_a"][1] and a["infinity_b"][1]
        assert not a["g1_k"][[3, 4, 5, 9, 10, 11].index(9)].any() and not c.vk["k"][1].any()


def test_an_honest_key_audits_to_zero_without_a_seed(ctx):
    c = case_of(ctx, (5, 1))
    assert audit_streams(ctx, c, seed=None) == 0


@pytest.mark.parametrize("n_com", [0, 2])
def test_a_phase2_state_audits_to_zero_before_and_after_contributions(ctx, n_com):
    """gamma = 1, delta = 1, then two contributions with sigma factors; the SRS as host rows and as a phase-1 state; the claim follows
    the state it borrows"""
    c = case_of(ctx, (100, n_com))
    sigma = [fr_arr([x])[0] for x in c.s["sigma"]]
    st = ctx.phase2_init(c.r1cs, c.srs, sigma)
    p1 = ctx.phase1_from_srs(c.srs, c.N)
    cl = ctx.key_claim_from_phase2(st)
    try:
        assert ctx.key_audit(c.r1cs, cl, srs=c.srs, seed=SEED) == 0
        assert ctx.key_audit(c.r1cs, cl, p1=p1, seed=SEED) == 0
        rng = P.SplitMix64(77)
        for _ in range(2):
            ctx.phase2_contribute(st, fr_arr([rng.fr()])[0], [fr_arr([rng.fr()])[0] for _ in range(n_com)] if n_com else None)
        assert ctx.key_audit(c.r1cs, cl, srs=c.srs, seed=SEED2) == 0
        assert ctx.key_audit(c.r1cs, cl, p1=p1, seed=SEED2) == 0
        pk, vk = ctx.phase2_to_streams(st, COMPRESSED)
        assert audit_streams(ctx, c, streams=(pk, vk)) == 0
    finally:
        ctx.key_claim_free(cl)
        ctx.phase1_free(p1)
        ctx.phase2_free(st)


# ---------------------------------------------------------------------------------------------------- 2: the sums against the model
def test_the_sums_of_every_relation_are_the_model_s(ctx):
    """N = 8, one commitment: pins the coefficient indexing, the class masks, the slot gathers, the bit reversal and the transform's
    orientation (the model transforms by the definition, index i = w^i)"""
    c = case_of(ctx, (5, 1))
    assert c.N == 8 and audit_streams(ctx, c) == 0
    got = ctx.key_audit_sums()
    s = c.s
    key = KR.honest_key(c.r1cs, s["tau"], s["alpha"], s["beta"], s["gamma"], s["delta"], s["sigma"])
    assert [int(x) for x in key["inf_a"]] == [int(x) for x in c.arrays["infinity_a"]]
    want = KR.sum_points(KR.sums(c.r1cs, KR.srs_exps(s["tau"], s["alpha"], s["beta"], 8), key, SEED))
    for name in ("a", "b1", "k_private", "k_public", "basis", "z"):
        assert g1_pts(got[name]) == list(want[name]), name
        assert want[name][0] is not None
    assert g2_pts(got["b2"]) == list(want["b2"])
    assert [tuple(g1_pts(p)) for p in got["sigma"]] == want["sigma"]
    # the two sides are equal where the relation compares points, and differ by gamma / delta where it pairs
    assert want["a"][0] == want["a"][1] and want["k_private"][0] != want["k_private"][1]


# ---------------------------------------------------------------------------------------------------- 3: tampers
def other_point(k):
    return P.g1_mul(P.G1_GEN, 1000 + k)


def tampered(c, name):
    """(arrays, vk) of case c with the tamper applied to copies"""
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.arrays.items()}
    a["ped"] = [(b.copy(), e.copy()) for b, e in c.arrays["ped"]]
    vk = {k: v.copy() for k, v in c.vk.items()}
    if name == "one point of A":
        a["g1_a"][1] = g1_arr([other_point(1)])[0]
    elif name == "a cancelling pair in A":
        E = other_point(2)
        p0, p2 = g1_pts(a["g1_a"][[0, 2]])
        a["g1_a"][0], a["g1_a"][2] = g1_arr([P.g1_add(p0, E)])[0], g1_arr([P.g1_add(p2, P.g1_neg(E))])[0]
    elif name == "a wire of A flagged infinite":
        j = int(np.nonzero(a["infinity_a"] == 0)[0][1])
        a["infinity_a"][j] = 1
        a["g1_a"] = np.delete(a["g1_a"], 1, axis=0)
    elif name == "one point of G2.B":
        a["g2_b"][0] = g2_arr([P.g2_mul(P.G2_GEN, 77)])[0]
    elif name == "K scaled":
        a["g1_k"] = g1_arr([None if p is None else P.g1_mul(p, 3) for p in g1_pts(a["g1_k"])])
    elif name == "one point of vk.K":
        vk["k"][0] = g1_arr([other_point(3)])[0]
    elif name == "two points of Z swapped":
        a["g1_z"][[0, 1]] = a["g1_z"][[1, 0]]
    elif name == "another delta":
        a["delta1"], a["delta2"] = g1_arr([P.g1_mul(P.G1_GEN, 4242)])[0], g2_arr([P.g2_mul(P.G2_GEN, 4242)])[0]
    elif name == "one point of Basis":
        a["ped"][0][0][0] = g1_arr([other_point(4)])[0]
    elif name == "BasisExpSigma of another sigma":
        a["ped"][0] = (a["ped"][0][0], g1_arr([None if p is None else P.g1_mul(p, 11) for p in g1_pts(a["ped"][0][0])]))
    else:
        raise KeyError(name)
    return a, vk


TAMPERS = [("one point of A", KR.A), ("a cancelling pair in A", KR.A), ("a wire of A flagged infinite", KR.A), ("one point of G2.B", KR.B2),
           ("K scaled", KR.K_PRIVATE), ("one point of vk.K", KR.K_PUBLIC), ("two points of Z swapped", KR.Z), ("another delta", KR.SMALL | KR.K_PRIVATE | KR.Z),
           ("one point of Basis", KR.BASIS | KR.SIGMA), ("BasisExpSigma of another sigma", KR.SIGMA)]


@pytest.mark.parametrize("tamper,bits", TAMPERS, ids=[t for t, _ in TAMPERS])
@pytest.mark.parametrize("name", [(5, 1), (100, 2)], ids=str)
def test_every_tamper_gives_exactly_its_mask(ctx, name, tamper, bits):
    c = case_of(ctx, name)
    a, vk = tampered(c, tamper)
    assert audit_arrays(ctx, c, arrays=a, vk=vk) == bits
    assert audit_arrays(ctx, c, arrays=a, vk=vk, seed=SEED2) == bits


@pytest.mark.parametrize("cls,bits", [(KR.CLS_P, KR.A | KR.K_PRIVATE), (KR.CLS_V, KR.A | KR.K_PUBLIC), (KR.CLS_C, KR.A | KR.BASIS)])
def test_the_key_of_the_circuit_with_another_coefficient(ctx, cls, bits):
    """the key mi_groth16_setup makes for the same circuit with one coefficient of A changed, at a wire of each class"""
    c = case_of(ctx, (100, 1))
    classes = KR.wire_classes(c.r1cs)
    rp, col, cf = c.r1cs["A"]
    e = next(i for i in range(len(col)) if classes[int(col[i])] == cls and int(col[i]) != c.r1cs["hot"])
    cf2 = cf.copy()
    cf2[e] = (int(cf[e]) + 1) % len(c.r1cs["coeffs"])
    other = dict(c.r1cs, A=(rp, col, cf2))
    pk, vk, _, _, _ = ctx.setup_to_streams(other, trapdoor(c.s), COMPRESSED, build=False)
    assert audit_streams(ctx, c, streams=(pk, vk)) == bits


def test_an_srs_of_another_tau_fails_all_but_small_and_sigma(ctx):
    c = case_of(ctx, (100, 1))
    srs = make_srs(ctx, c.N, (c.s["tau"] + 1) % R, c.s["alpha"], c.s["beta"])
    assert audit_streams(ctx, c, srs=srs) == KR.ALL & ~(KR.SMALL | KR.SIGMA)


# ---------------------------------------------------------------------------------------------------- 4: refusals
SHAPES = [("n_z", {"g1_z": 7}, None), ("nb_wires", {"nb_wires": 49}, None), ("n_a", {"g1_a": -1}, None), ("n_b", {"g1_b": -1}, None),
          ("n_g2_b", {"g2_b": -1}, None), ("n_k", {"g1_k": -1}, None), ("vk.n_k", {"vk_k": -1}, None), ("n_ped", {}, 0), ("n_basis[0]", {"basis0": -1}, None)]


@pytest.mark.parametrize("count,change,n_ped", SHAPES, ids=[s[0] for s in SHAPES])
def test_a_claim_of_another_shape_is_refused_naming_the_count(ctx, count, change, n_ped):
    B = load_binding()
    c = case_of(ctx, (5, 1))
    assert audit_arrays(ctx, c) == 0   # the workspaces have grown
    a = dict(c.arrays)
    own = {"g1_z": len(a["g1_z"]), "g1_a": len(a["g1_a"]), "g1_b": len(a["g1_b"]), "g2_b": len(a["g2_b"]), "g1_k": len(a["g1_k"]), "vk_k": len(c.vk["k"]),
           "basis0": len(a["ped"][0][0]), "nb_wires": a["nb_wires"]}
    counts = {k: (v if v > 0 else own[k] + v) for k, v in change.items()}
    if "nb_wires" in counts:
        a["infinity_a"] = np.append(a["infinity_a"], np.uint8(1)); a["infinity_b"] = np.append(a["infinity_b"], np.uint8(1))
    before = ctx.mem_ledger()
    with ArrayClaim(ctx, a, c.vk, c.vk_ped, counts=counts, n_ped=n_ped) as cl:
        with pytest.raises(B.MiError) as ei:
            ctx.key_audit(c.r1cs, cl.h, srs=c.srs, seed=SEED)
    assert "rc=-1" in str(ei.value) and "key audit: claim." + count + " is" in str(ei.value), str(ei.value)
    assert ctx.mem_ledger() == before


def test_other_refusals(ctx):
    B = load_binding()
    c = case_of(ctx, (5, 1))
    assert audit_streams(ctx, c) == 0 and audit_arrays(ctx, c) == 0
    before = ctx.mem_ledger()

    def refused(text, f):
        with pytest.raises(B.MiError) as ei:
            f()
        assert "rc=-1" in str(ei.value) and text in str(ei.value), str(ei.value)
        assert ctx.mem_ledger() == before

    h = ctx.key_claim_from_streams(*c.streams[COMPRESSED])
    p1 = ctx.phase1_from_srs(c.srs, c.N)
    try:
        refused("exactly one of srs and p1", lambda: ctx.key_audit(c.r1cs, h, srs=c.srs, p1=p1, seed=SEED))
        refused("exactly one of srs and p1", lambda: ctx.key_audit(c.r1cs, h, seed=SEED))
        refused("unknown flag", lambda: ctx.key_audit(c.r1cs, h, srs=c.srs, seed=SEED, flags=4))
        bad = dict(c.srs, tau_g1=c.srs["tau_g1"].copy())
        bad["tau_g1"][3] = 0
        refused("phase2: srs.tau_g1[3] is at infinity or not on its curve", lambda: ctx.key_audit(c.r1cs, h, srs=bad, seed=SEED))
        refused("phase2: srs.n_tau_g1 is 15, the circuit needs 16 points", lambda: ctx.key_audit(c.r1cs, h, srs=dict(c.srs, n_tau_g1=15), seed=SEED))
        out = dict(c.srs, tau_g2=c.srs["tau_g2"].copy())
        out["tau_g2"][2] = g2_arr([V.twist_point_outside_subgroup()])[0]
        refused("phase2: srs.tau_g2[2] is not in the r-torsion", lambda: ctx.key_audit(c.r1cs, h, srs=out, seed=SEED))
        big = case_of(ctx, (100, 1))   # a circuit above the phase-1 state's domain
        hb = ctx.key_claim_from_streams(*big.streams[COMPRESSED])
        try:
            refused("the circuit needs 256 points", lambda: ctx.key_audit(big.r1cs, hb, p1=p1, seed=SEED))
        finally:
            ctx.key_claim_free(hb)
        far = dict(c.r1cs, A=(c.r1cs["A"][0], c.r1cs["A"][1] + np.uint32(1000), c.r1cs["A"][2]))
        refused("key audit: A", lambda: ctx.key_audit(far, h, srs=c.srs, seed=SEED))
    finally:
        ctx.phase1_free(p1)
        ctx.key_claim_free(h)
    # the points of plain arrays
    a = dict(c.arrays, g1_k=c.arrays["g1_k"].copy())
    a["g1_k"][2][0] ^= np.uint64(1)
    refused("key claim: desc.g1_k[2] is not a point of its curve", lambda: ArrayClaim(ctx, a, c.vk, c.vk_ped))
    a = dict(c.arrays, g2_b=c.arrays["g2_b"].copy())
    a["g2_b"][1] = g2_arr([V.twist_point_outside_subgroup()])[0]
    refused("key claim: desc.g2_b[1] is not in the r-torsion", lambda: ArrayClaim(ctx, a, c.vk, c.vk_ped))
    a = dict(c.arrays, g1_a=c.arrays["g1_a"].copy())
    a["g1_a"][0] = 0
    refused("key claim: desc.g1_a[0] is not a point of its curve or is at infinity", lambda: ArrayClaim(ctx, a, c.vk, c.vk_ped))
    refused("key claim: desc.delta1 is at infinity", lambda: ArrayClaim(ctx, dict(c.arrays, delta1=np.zeros(8, np.uint64)), c.vk, c.vk_ped))
    # a stream is refused by the loaders' own code, with their texts
    pk, vk = c.streams[COMPRESSED]
    info, _ = B.pk_stream_inspect(pk)
    broken = bytearray(pk)
    broken[info.off_g1_k:info.off_g1_k + 32] = b"\xbf" + b"\xff" * 31   # x >= p
    refused("keyfile: G1.K[0] is malformed", lambda: ctx.key_claim_from_streams(bytes(broken), vk))
    refused("vkfile: the stream has neither the layout", lambda: ctx.key_claim_from_streams(pk, vk[:-3]))
