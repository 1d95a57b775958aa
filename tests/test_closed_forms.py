"""CPU pins of tests/closed_forms.py: every closed form equals pyref / cref at 2^4..2^12, in all 8 NTT modes and with its plants, and
every checker rejects a correct result with one limb of one output changed or two outputs swapped (at a random slot and at a chunk
boundary).  Small chunk sizes make the chunked paths cross many chunk boundaries at these sizes."""
import numpy as np
import pytest
import pyref as P
import cref
import closed_forms as CF
from helpers import fr_arr, fr_vals, g1_pts, g2_pts, g1_from_jac, g2_from_jac

Y = 0x1234_5678_9ABC_DEF0_1357_9BDF_2468_ACE0_0F1E_2D3C_4B5A_6978_8796_A5B4_C3D2_E1F0 % P.R_MOD


def _plants(log_n):
    N = 1 << log_n
    pl = CF.ntt_plants(log_n, seed=log_n)
    # at these sizes the 2^10 / 2^20 boundaries are mostly out of range: add chunk-boundary and odd positions
    return sorted(dict(pl + [(p, 7 + p) for p in (3, N // 4, N // 4 - 1, N - 2) if 0 <= p < N]).items())


def _ref_ntt(a, log_n, flags):
    dom = P.Domain(1 << log_n)
    dec = P.DIT if flags & CF.DIT else P.DIF
    f = P.fft_inverse if flags & CF.INVERSE else P.fft
    return fr_arr(f(dom, fr_vals(a), dec, coset=bool(flags & CF.COSET)))


def _mutants(out, chunk_bits):
    """a correct vector with one limb of one row changed, or two rows swapped: at a random row and at a chunk boundary"""
    rng = np.random.default_rng(len(out))
    m = 1 << min(chunk_bits, len(out).bit_length() - 1)
    for i in (int(rng.integers(0, len(out))), m % len(out), (m - 1) % len(out)):
        x = out.copy()
        x[i, int(rng.integers(0, 4))] ^= np.uint64(int(rng.integers(1, 1 << 63)))
        yield "limb", i, x
        j = (i + 1 + int(rng.integers(0, len(out) - 1))) % len(out)
        if not np.array_equal(out[i], out[j]):
            x = out.copy()
            x[[i, j]] = x[[j, i]]
            yield "swap", i, x


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("log_n", [4, 7, 12])
def test_ntt_closed_form_equals_pyref(log_n, flags):
    cb = max(2, log_n - 3)
    pl = _plants(log_n)
    a = CF.ntt_input(log_n, flags, Y, pl, chunk_bits=cb)
    # the input really is y^i (+ deltas) at the slots the mode reads
    dit = flags & CF.DIT
    N = 1 << log_n
    want_in = [(pow(Y, i, P.R_MOD) + dict(pl).get(i, 0)) % P.R_MOD for i in range(N)]
    if dit:
        want_in = [want_in[P.bitrev(s, log_n)] for s in range(N)]
    assert fr_vals(a) == want_in
    out = cref.ntt(a, log_n, flags)
    if log_n <= 7:
        assert np.array_equal(out, _ref_ntt(a, log_n, flags))
    assert CF.ntt_check(out, log_n, flags, Y, pl, chunk_bits=cb) == []
    for kind, i, bad in _mutants(out, cb):
        assert CF.ntt_check(bad, log_n, flags, Y, pl, chunk_bits=cb), f"{kind} at {i} passed"


@pytest.mark.parametrize("flags", [0, 1, 2 | 4, 1 | 2 | 4])
def test_ntt_checker_rejects_other_modes_and_inputs(flags):
    """a right transform of the wrong mode or of a slightly different input fails: the checker pins the conventions, not just a shape"""
    log_n, cb = 8, 5
    pl = _plants(log_n)
    a = CF.ntt_input(log_n, flags, Y, pl, chunk_bits=cb)
    for other in range(8):
        if other != flags:
            assert CF.ntt_check(cref.ntt(a, log_n, other), log_n, flags, Y, pl, chunk_bits=cb)
    a2 = a.copy()
    a2[[1, 2]] = a2[[2, 1]]
    assert CF.ntt_check(cref.ntt(a2, log_n, flags), log_n, flags, Y, pl, chunk_bits=cb)
    pl2 = [(p + (1 if i == len(pl) - 2 else 0), d) for i, (p, d) in enumerate(pl)]   # one plant a row off
    assert CF.ntt_check(cref.ntt(a, log_n, flags), log_n, flags, Y, pl2, chunk_bits=cb)


@pytest.mark.parametrize("log_n", [4, 8, 12])
def test_compute_h_closed_form_equals_cref(log_n):
    ta, tb = CF.compute_h_poly(log_n, seed=log_n)
    a = CF.poly_eval(log_n, ta, chunk_bits=max(2, log_n - 2))
    b = CF.poly_eval(log_n, tb, chunk_bits=max(2, log_n - 2))
    N = 1 << log_n
    w = P.Domain(N).gen
    for i in (0, 1, N - 1):
        assert fr_vals(a[i:i + 1])[0] == sum(c * pow(w, i * d, P.R_MOD) for d, c in ta) % P.R_MOD
    c = cref.field_op(0, CF.MUL, a, b)
    h = cref.compute_h(log_n, a, b, c)
    assert CF.compute_h_check(h, log_n, ta, tb) == []
    assert len(CF.compute_h_expected(log_n, ta, tb)) >= 3
    for kind, i, bad in _mutants(h, log_n - 2):
        assert CF.compute_h_check(bad, log_n, ta, tb), f"{kind} at {i} passed"
    # unreversed h, or the polynomial of a plant one degree off, fails
    assert CF.compute_h_check(h[CF.bitrev_bits(np.arange(N), log_n)], log_n, ta, tb)
    assert CF.compute_h_check(h, log_n, [(d - 1 if k == 0 else d, cf) for k, (d, cf) in enumerate(ta)], tb)


def _msm_case(n, kind, g2=False):
    x = 0xABCDEF0123456789 * 0x1000000000000000000000001 % P.R_MOD
    plants = CF.msm_plants(n, boundaries=(n // 2, 16), seed=n)
    if kind == "geo":
        return CF.MsmCase(n, x, y=Y, plants=plants)
    return CF.MsmCase(n, x, mix=CF.mix_values(37, 300, 200, 100, seed=n), plants=plants)


@pytest.mark.parametrize("kind", ["geo", "mix"])
@pytest.mark.parametrize("log_n,g2", [(4, False), (8, False), (12, False), (4, True), (8, True)], ids=["g1-4", "g1-8", "g1-12", "g2-4", "g2-8"])
def test_msm_closed_form_equals_cref(log_n, g2, kind):
    n = (1 << log_n) - (log_n & 1)
    case = _msm_case(n, kind)
    e = np.concatenate([r for _, r in case.chunks("e", chunk=1 << max(2, log_n - 3))])
    s = np.concatenate([r for _, r in case.chunks("s", chunk=1 << max(2, log_n - 3))])
    assert len(case.final) >= 10
    # rows are what they claim: x^i / y^i / mix, with the plants applied
    ev, sv = fr_vals(e), fr_vals(s)
    for r in list(case.final)[:12] + [0, n - 1, n // 3]:
        want = case.final.get(r, (case._e(r), case._s(r)))
        assert (ev[r], sv[r]) == want
    kinds = {k for k, _ in case.plants.values()}
    assert {"eq", "neg", "inf", "eqp", "sc"} <= kinds
    gen = CF.G2 if g2 else CF.G1
    pts = cref.batch_scalar_mul(gen, e, g2=g2)
    S = case.sum()
    if g2:
        assert g2_from_jac(cref.msm_g2(pts, s)) == P.g2_mul(P.G2_GEN, S)
    else:
        assert g1_from_jac(cref.msm_g1(pts, s)) == P.g1_mul(P.G1_GEN, S)
    assert S == sum(a * b for a, b in zip(ev, sv)) % P.R_MOD
    # a plant correction one row off changes the sum
    r0 = sorted(case.final)[len(case.final) // 2]
    off = CF.MsmCase(n, case.x, y=case.y, mix=case.mix, plants={(r0 + 1 if r == r0 else r): v for r, v in case.plants.items()})
    assert off.sum() != S


def test_msm_spot_rows_cover_plants_and_ends():
    case = _msm_case(1 << 10, "geo")
    rows = case.spot_rows()
    assert 0 in rows and (1 << 10) - 1 in rows and len(rows) == 64
    assert sum(r in case.final for r in rows) >= 16
