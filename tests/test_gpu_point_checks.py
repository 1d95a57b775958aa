"""GPU: which words each ceremony and audit entry point takes for a point -- a PIN of current behaviour, not an endorsement of it.

Every bulk check of plain affine points goes through csrc/point_check.cuh (k_points_check_g1 / _g2) under one of three rules.  This file
records, entry point by entry point, what the library did BEFORE those rules were written down in one place, so that a later change of
a rule is a deliberate change of one of the verdicts below:

    input                                        x + q (words not reduced)   off the curve   (0, 0)
    an SRS row into mi_phase2_init               ACCEPTED                    refused         refused
    an SRS row into mi_phase1_from_srs           ACCEPTED                    refused         refused
    claim.g1_z into mi_phase2_verify_adopt       refused                     refused         passes the point check (then MI_PHASE2_BAD_Z)
    claim.basis_exp_sigma[k] into ..._sigma      refused                     refused         passes the point check (then MI_PHASE2_BAD_BES)
    desc.g1_k into mi_key_claim_from_arrays      refused                     refused         accepted (the array may hold it)
    desc.g2_b into mi_key_claim_from_arrays      refused                     refused         refused

"x + q": the four words of the point's x (x.a0 on the twist), Montgomery form, read as a 256-bit integer, plus the base field's
modulus: a second encoding of the same element (csrc/pairing.cuh says why a verifier wants one).  An SRS row is not asked for reduced
words; nobody chose that.  A refusal names the index; an index >= 256 puts the bad point into a second workgroup of each kernel."""
import numpy as np
import pytest
import cref
import pyref as P
import setup_cases as S
import test_gpu_phase2 as T2
import test_gpu_phase2_check as TG
import test_gpu_phase2_sigma as TS
import test_gpu_keyaudit as KA
from helpers import fr_arr, g1_arr, g2_arr
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
R, Q = P.R_MOD, P.Q_MOD
NC = 300    # N = 512: tau_g1 holds 1024 points, tau_g2 and Z 512


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def with_point(arr, i, how):
    """a copy of a (n, 8) or (n, 16) array of points with point i replaced: "x + q", "off curve" or "infinity\""""
    out = arr.copy()
    g2 = arr.shape[1] == 16
    if how == "x + q":
        x = cref.limbs_to_int(out[i][:4]) + Q
        assert Q <= x < 1 << 256
        out[i][:4] = cref.int_to_limbs(x)
    elif how == "off curve":
        out[i] = g2_arr([((1, 2), (3, 4))])[0] if g2 else g1_arr([(1, 3)])[0]
    elif how == "infinity":
        out[i] = 0
    else:
        raise KeyError(how)
    return out


@pytest.fixture(scope="module")
def ceremony(ctx):
    """one circuit with one commitment (N = 512), its SRS, a contributor after one proved delta step and one proved sigma step, the two
    claims it hands over, and a verifier's fresh state"""
    B = load_binding()
    tau, alpha, beta, sigma = T2.secrets(2600, 1)
    r1cs = S.synth_r1cs(NC, nb_wires=NC + 40, nb_public=5, seed=2601, per_row=4, n_coeffs=64, n_heavy=2, heavy_len=40, n_empty_cols=6, commitments=1, n_committed=4)
    srs = T2.make_srs(ctx, NC, tau, alpha, beta)
    sg = [fr_arr([x])[0] for x in sigma]
    c, v = ctx.phase2_init(r1cs, srs, sg), ctx.phase2_init(r1cs, srs, sg)
    rec = ctx.phase2_contribute_proved(c, fr_arr([TG.D1])[0], fr_arr([TG.K1])[0])
    claim = TG.claim_of(ctx, B, c, TG.D1)
    step, h = ctx.phase2_contribute_sigma_proved(c, fr_arr(TS.S1[:1]), fr_arr(TS.N1[:1]))
    sclaim = TS.sigma_claim_of(ctx, B, c, 1)
    yield {"r1cs": r1cs, "srs": srs, "sg": sg, "v": v, "rec": rec, "claim": claim, "step": step, "h": h, "sclaim": sclaim}
    ctx.phase2_free(c); ctx.phase2_free(v)


def refused(B, text, f):
    with pytest.raises(B.MiError) as ei:
        f()
    assert "rc=-1" in str(ei.value) and text in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------------------------------- SRS rows
SRS_ROWS = [("tau_g1", 300), ("alpha_tau_g1", 7), ("tau_g2", 300)]


@pytest.mark.parametrize("row,i", SRS_ROWS, ids=[r for r, _ in SRS_ROWS])
def test_srs_rows_into_phase2_init(ctx, ceremony, row, i):
    B = load_binding()
    cer = ceremony
    assert len(cer["srs"][row]) > i
    st = ctx.phase2_init(cer["r1cs"], dict(cer["srs"], **{row: with_point(cer["srs"][row], i, "x + q")}), cer["sg"])   # ACCEPTED
    ctx.phase2_free(st)
    for how in ("off curve", "infinity"):
        bad = dict(cer["srs"], **{row: with_point(cer["srs"][row], i, how)})
        refused(B, f"phase2: srs.{row}[{i}] is at infinity or not on its curve", lambda: ctx.phase2_init(cer["r1cs"], bad, cer["sg"]))


@pytest.mark.parametrize("row,i", SRS_ROWS, ids=[r for r, _ in SRS_ROWS])
def test_srs_rows_into_phase1_from_srs(ctx, ceremony, row, i):
    B = load_binding()
    srs, N = ceremony["srs"], T2.domain_size(NC)
    p1 = ctx.phase1_from_srs(dict(srs, **{row: with_point(srs[row], i, "x + q")}), N)   # ACCEPTED
    ctx.phase1_free(p1)
    for how in ("off curve", "infinity"):
        bad = dict(srs, **{row: with_point(srs[row], i, how)})
        refused(B, f"phase2: srs.{row}[{i}] is at infinity or not on its curve", lambda: ctx.phase1_from_srs(bad, N))


# ---------------------------------------------------------------------------------------------------- claimed states
def test_claimed_z_into_verify_adopt(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    before = ctx.phase2_to_streams(cer["v"], T2.RAW)
    for i, how in ((300, "x + q"), (300, "off curve"), (3, "x + q")):
        bad = dict(cer["claim"], g1_z=with_point(cer["claim"]["g1_z"], i, how))
        refused(B, f"phase2 verify: claim.g1_z[{i}] is not a point of the curve", lambda: TG.adopt(ctx, cer["v"], bad, [cer["rec"]]))
    inf = dict(cer["claim"], g1_z=with_point(cer["claim"]["g1_z"], 300, "infinity"))
    assert TG.adopt(ctx, cer["v"], inf, [cer["rec"]]) == (B.PHASE2_BAD_Z, 1)    # infinity is a point here; the relation then fails
    assert ctx.phase2_to_streams(cer["v"], T2.RAW) == before


def test_claimed_basis_exp_sigma_into_verify_adopt_sigma(ctx, ceremony):
    B = load_binding()
    cer = ceremony
    bes = cer["sclaim"]["bes"][0]
    before = ctx.phase2_to_streams(cer["v"], T2.RAW)
    for how in ("x + q", "off curve"):
        bad = dict(cer["sclaim"], bes=[with_point(bes, 2, how)])
        refused(B, "phase2 verify sigma: claim.basis_exp_sigma[0][2] is not a point of the curve", lambda: TS.adopt_sigma(ctx, cer["v"], bad, [cer["step"]], [cer["h"]]))
    inf = dict(cer["sclaim"], bes=[with_point(bes, 2, "infinity")])
    assert TS.adopt_sigma(ctx, cer["v"], inf, [cer["step"]], [cer["h"]]) == (B.PHASE2_BAD_BES, 1, 1)
    assert ctx.phase2_to_streams(cer["v"], T2.RAW) == before


# ---------------------------------------------------------------------------------------------------- the arrays of a key claim
def test_arrays_into_key_claim_from_arrays(ctx):
    B = load_binding()
    c = KA.case_of(ctx, (5, 1))
    assert len(c.arrays["g1_k"]) > 2 and len(c.arrays["g2_b"]) > 2
    for how in ("x + q", "off curve"):
        a = dict(c.arrays, g1_k=with_point(c.arrays["g1_k"], 2, how))
        refused(B, "key claim: desc.g1_k[2] is not a point of its curve", lambda: KA.ArrayClaim(ctx, a, c.vk, c.vk_ped))
    with KA.ArrayClaim(ctx, dict(c.arrays, g1_k=with_point(c.arrays["g1_k"], 2, "infinity")), c.vk, c.vk_ped) as cl:   # K may hold infinity
        assert cl.h is not None
    for how in ("x + q", "off curve", "infinity"):
        a = dict(c.arrays, g2_b=with_point(c.arrays["g2_b"], 1, how))
        refused(B, "key claim: desc.g2_b[1] is not a point of its curve or is at infinity", lambda: KA.ArrayClaim(ctx, a, c.vk, c.vk_ped))
