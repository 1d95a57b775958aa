"""GPU: the sizes the C-ABI accepts above 2^26, against the closed forms of tests/closed_forms.py (the oracle takes minutes there).

  G1 MSM    n = 2^27 - 1 (the LDS-staged two-pass sort, 16 n < 2^31) and n = 2^27 (the one-pass sort with 2^31 entries), points [x^i]G
            built on the device, full-width y^i scalars and the census mix, planted equal / opposite / infinity / edge rows
  NTT       all 8 flag combinations at 2^27 (the {10, 10, 8} radix plan): one full closed-form check per (inverse, coset) class, and the
            DIT transform of the same logical input equal to the DIF one bit-reversed
  computeH  2^28, with c given and c = NULL (formed on the device)
  caps      a key whose per-device MSMs would exceed 2^27 pairs is refused at load, an MSM of 2^27 + 1 pairs is refused, and the
            context then proves a small key correctly
  proof     N = 2^27 with a key of known discrete logs: checked in the exponent, or refused with MI_ENOMEM on a device too small for it

Left out to keep the suite's time: the NTT at 2^28 (computeH at 2^28 runs its coset DIT, inverse and inverse coset transforms) and the
G2 MSM at 2^27.

Each test trims the context first, frees what it allocates, and prints its phase times, the context's device ledger and the process's
host peak RSS.
"""
import ctypes as C
import os
import resource
import sys
import time
import numpy as np
import pytest
import pyref as P
import cref
import closed_forms as CF
import dlog_keys as D
from helpers import g1_pts, g1_from_jac
from gpu_common import load_binding

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wire_census  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 27
X = 0x0DDBA11_5EED_CAFE_F00D_BEEF_1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321 % P.R_MOD
Y = 0x1234_5678_9ABC_DEF0_1357_9BDF_2468_ACE0_0F1E_2D3C_4B5A_6978_8796_A5B4_C3D2_E1F0 % P.R_MOD


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


class Phases:
    def __init__(self, name):
        self.name, self.t, self.parts = name, time.perf_counter(), []

    def __call__(self, label):
        now = time.perf_counter()
        self.parts.append(f"{label} {now - self.t:.1f} s")
        self.t = now

    def report(self, ctx, held_gb=0.0):
        led = ctx.mem_ledger()
        rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6
        print(f"{self.name}: {', '.join(self.parts)}; device: test buffers {held_gb:.1f} GB, context "
              f"{sum(v for k, v in led.items() if k.startswith('ctx')):.1f} GB {led}; host peak RSS {rss:.1f} GB")


def _upload_at(ctx, dev, row0, rows, width=4):
    rows = np.ascontiguousarray(rows, np.uint64)
    ctx._ck(ctx.lib.mi_dev_upload(ctx.h, C.c_void_p(dev.ptr + 8 * width * row0), rows.ctypes.data_as(C.c_void_p), C.c_size_t(rows.nbytes)))


def _download_rows(ctx, dev, rows, width):
    out = np.zeros((len(rows), width), np.uint64)
    for k, r in enumerate(rows):
        ctx._ck(ctx.lib.mi_dev_download(ctx.h, out[k].ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr + 8 * width * int(r)), C.c_size_t(8 * width)))
    return out


# ---------------------------------------------------------------------------------------------------- caps (cheap, first)
def _desc(log_n, nb_wires, n_z):
    """a key header that is inconsistent on purpose beyond the size (no A points for wires the masks put in A): without the load-time cap
    it is still refused, by the count check, before any point is read"""
    z8 = np.zeros(8, np.uint64)
    z16 = np.zeros(16, np.uint64)
    return {"log_n": log_n, "nb_public": 1, "nb_wires": nb_wires, "infinity_a": np.zeros(nb_wires, np.uint8), "infinity_b": np.ones(nb_wires, np.uint8),
            "g1_a": (0, 0), "g1_b": (0, 0), "g1_k": (0, 0), "g1_z": (0, n_z), "g2_b": (0, 0),
            "alpha1": z8, "beta1": z8, "delta1": z8, "beta2": z16, "delta2": z16}


def test_oversized_keys_refused_at_load_then_small_proof(ctx):
    B = load_binding()
    ctx.trim()
    ph = Phases("caps")
    before = ctx.mem_ledger()
    for log_n, nb_wires in ((28, 1000), (10, CAP + 1)):
        with pytest.raises(B.MiError) as ei:
            ctx.pk_load(_desc(log_n, nb_wires, (1 << log_n) - 1), device_points=True)
        msg = str(ei.value)
        assert "2^27" in msg and "mi_pk_load_sharded" in msg, msg
    assert ctx.mem_ledger() == before
    ph("refusals")
    # the context is still good: a small key from known exponents proves right
    e = D.make_exps(12, 4000, 17, 64, (900, 500), True, 1227)
    W = D.witness(e, 1, 1237)
    a, b, c = D.constraint_values(4000, 1, 1247)
    r, s = cref.gen_scalars(2, 1257, 0)
    pkh = ctx.pk_load(D.points_from_exps(e, ctx))
    try:
        got, _ = ctx.prove(pkh, W, a, b, None, r, s)
    finally:
        ctx.pk_free(pkh)
    D.check_proof(got, D.expected_proof_exps(e, W, a, b, r, s))
    ph("2^12 proof")
    ph.report(ctx)


# ---------------------------------------------------------------------------------------------------- whole proof at 2^27, in the exponent
def test_prove_2p27_census_dlog_keys(ctx):
    """N = 2^27 (the largest key one device takes: Z has 2^27 - 1 pairs), nbPublic 4097, N / 32 committed wires, N - 100 constraints
    (the fused padding), census masks and witness mix, all plants; the key built on the device, the production table plan, c formed
    on the device.  The proof is checked in the exponent (tests/dlog_keys.py, chunked) -- or, where the device cannot hold the key and
    the five MSMs' workspaces (a 288 GB MI355X cannot: DESIGN.md 3), the prove must refuse with MI_ENOMEM and leave the context working:
    the next calls on it, a 2^12 proof among them, must succeed"""
    B = load_binding()
    ctx.trim()
    L, N = 27, 1 << 27
    ph = Phases("proof 2^27")
    masks = wire_census.census_masks_permille()
    dist = B.dist_mix(*wire_census.census_mix_permille())
    seed = 2727
    e = D.make_exps(L, N - 1000, 4097, N >> 5, masks, True, seed)
    ph("exponents")
    pk, bufs = D.points_from_exps(e, ctx, device=True)
    held = sum(d.nbytes for d in bufs) / 1e9
    ph("key points on the device (spot-checked)")
    got, err = None, None
    try:
        pkh = ctx.pk_load(pk, device_points=True)
        del pk
        ph("pk_load")
        try:
            key_gb = sum(v for k, v in ctx.mem_ledger(pkh).items() if k.startswith("key"))
            print(f"N=2^27 census masks {masks}: pk_table_plan (c_ak, c_b, c_z) = {ctx.pk_table_plan(pkh)}, key {key_gb:.1f} GB "
                  f"(+ {held:.1f} GB of adopted point arrays)")
            W = D.witness(e, dist, seed + 10)
            a = cref.gen_scalars(N - 100, seed + 20, dist)
            b = cref.gen_scalars(N - 100, seed + 21, 0)
            r, s = cref.gen_scalars(2, seed + 30, 0)
            ph("witness and constraints")
            try:
                got, st = ctx.prove(pkh, W, a, b, None, r, s)
                ph(f"prove ({st['total_ms']:.0f} ms)")
            except B.MiError as x:
                err = str(x)
                ph("prove refused")
            ph.report(ctx, held + key_gb)
        finally:
            ctx.pk_free(pkh)
    finally:
        for d in bufs:
            d.free()
    ctx.trim()
    if got is None:
        print(f"N=2^27 single-device prove: {err}")
        assert "rc=-3" in err and "out of memory" in err, err     # MI_ENOMEM, nothing else
        del W, a, b
        # the context is whole again: a 2^12 proof on it is right
        e2 = D.make_exps(12, 4000, 17, 64, (900, 500), True, 2712)
        W2 = D.witness(e2, dist, 2713)
        a2, b2, _ = D.constraint_values(4000, dist, 2714)
        r2, s2 = cref.gen_scalars(2, 2715, 0)
        pkh = ctx.pk_load(D.points_from_exps(e2, ctx))
        try:
            got2, _ = ctx.prove(pkh, W2, a2, b2, None, r2, s2)
        finally:
            ctx.pk_free(pkh)
        D.check_proof(got2, D.expected_proof_exps(e2, W2, a2, b2, r2, s2))
        ph("2^12 proof after the refusal")
    else:
        D.check_proof(got, D.expected_proof_exps(e, W, a, b, r, s))
        ph("exponent reference")
    ph.report(ctx)


# ---------------------------------------------------------------------------------------------------- MSM at 2^27 - 1 and 2^27
def _slice_boundaries(n):
    """one-pass sort slices (64 of ceil(n / 64)), two-pass sort slices of 512 scalars, around the first and the last"""
    per = (n + 63) // 64
    return tuple(sorted({per, 2 * per, 63 * per, 512, 1024, n - 512, n >> 1}))


@pytest.fixture(scope="class")
def msm27(ctx):
    """exponents x^i (with the point plants) and their G1 points on the device, 2^27 + 1 rows (the last row for the refusal)"""
    ctx.trim()
    ph = Phases("MSM 2^27 points")
    n = CAP
    plants = CF.msm_plants(n, _slice_boundaries(n), seed=27)
    cases = {"geo": CF.MsmCase(n, X, y=Y, plants=plants),
             "mix": CF.MsmCase(n, X, mix=CF.mix_values(997, *wire_census.census_mix_permille(), seed=27), plants=plants)}
    exps = ctx.alloc(32 * (n + 1))
    for lo, rows in cases["geo"].chunks("e"):
        _upload_at(ctx, exps, lo, rows)
    _upload_at(ctx, exps, n, np.zeros((1, 4), np.uint64))
    ph("exponents")
    pts = ctx.alloc(64 * (n + 1))
    ctx.batch_scalar_mul_dev(CF.G1, exps.ptr, n + 1, pts.ptr)
    ctx.sync()
    ph("points")
    rows = cases["geo"].spot_rows(64, seed=27)
    got = g1_pts(_download_rows(ctx, pts, rows, 8))
    assert got == [P.g1_mul(P.G1_GEN, cases["geo"].final.get(r, (cases["geo"]._e(r), 0))[0]) for r in rows], "a point is not [x^i]G"
    ph("spot check")
    ph.report(ctx, (exps.nbytes + pts.nbytes) / 1e9)
    yield {"n": n, "cases": cases, "exps": exps, "pts": pts}
    exps.free()
    pts.free()


class TestMsm2p27:
    """the G1 MSMs share the 2^27 exponents and points of the class fixture, freed when the class is done"""

    @pytest.mark.parametrize("kind", ["geo", "mix"])
    def test_g1_msm_2p27_minus_1_and_2p27(self, ctx, msm27, kind):
        """n = 2^27 - 1 runs the two-pass sort, n = 2^27 the one-pass sort (2^31 digit entries); both against the closed form"""
        ctx.trim()
        ph = Phases(f"G1 MSM 2^27, {kind} scalars")
        n, case = msm27["n"], msm27["cases"][kind]
        sc = ctx.alloc(32 * (n + 1))
        try:
            for lo, rows in case.chunks("s"):
                _upload_at(ctx, sc, lo, rows)
            _upload_at(ctx, sc, n, CF.mont(1).reshape(1, 4))
            ph("scalars")
            S = case.sum()
            e_last, s_last = case.final.get(n - 1, (case._e(n - 1), case._s(n - 1)))
            for m, S_m, sort in ((n - 1, (S - e_last * s_last) % P.R_MOD, "two_pass"), (n, S, "one_pass")):
                c1, c2 = ctx.counter("generic_sorts_two_pass"), ctx.counter("generic_sorts_one_pass")
                got = ctx.msm_g1_dev(msm27["pts"].ptr, sc.ptr, m)
                ran = ("two_pass" if ctx.counter("generic_sorts_two_pass") > c1 else "") + ("one_pass" if ctx.counter("generic_sorts_one_pass") > c2 else "")
                ph(f"n = {m} ({ran} sort, {ctx.stats()['total_ms']:.0f} ms)")
                assert ran == sort
                assert g1_from_jac(got) == P.g1_mul(P.G1_GEN, S_m), f"G1 MSM of {m} pairs"
            B = load_binding()
            with pytest.raises(B.MiError, match="2\\^27"):
                ctx.msm_g1_dev(msm27["pts"].ptr, sc.ptr, n + 1)
            ph.report(ctx, (msm27["exps"].nbytes + msm27["pts"].nbytes + sc.nbytes) / 1e9)
        finally:
            sc.free()


# ---------------------------------------------------------------------------------------------------- NTT at 2^27
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["fwd", "inv", "coset", "inv-coset"])
def test_ntt_2p27_dif_and_dit_closed_form(ctx, flags):
    """the DIF transform checked against the closed form at every output; the DIT transform of the same logical input equals it
    bit-reversed, so both decimations are checked at every output"""
    ctx.trim()
    L = 27
    N = 1 << L
    ph = Phases(f"NTT 2^27 flags {flags} and {flags | 4}")
    pl = CF.ntt_plants(L, seed=flags)
    y = (Y + flags) % P.R_MOD
    buf = ctx.alloc(32 * N)
    try:
        outs = {}
        for f in (flags, flags | CF.DIT):
            for off, rows in CF.ntt_input_chunks(L, f, y, pl):
                _upload_at(ctx, buf, off, rows)
            ph(f"input {f}")
            ctx.ntt_dev(buf.ptr, L, f)
            ctx.sync()
            ph(f"ntt {f}")
            outs[f] = buf.download((N, 4))
            ph("download")
        bad = CF.ntt_check(outs[flags], L, flags, y, pl)
        ph("closed-form check")
        assert bad == [], f"flags {flags}: slots {bad[:8]} break the closed form"
        _, m, chunks, lo_rev = CF.chunking(L)
        row = np.dtype((np.void, 32))   # one 32-byte element per row: the gathers move whole rows
        dif, dit = outs[flags].view(row).reshape(N), outs[flags | CF.DIT].view(row).reshape(N)
        for h in range(chunks):
            slots = (lo_rev << (L - CF.CHUNK_BITS)) | int(CF.bitrev_bits(h, L - CF.CHUNK_BITS))
            assert np.array_equal(dit[h * m:(h + 1) * m], dif[slots]), f"flags {flags | 4}: DIT output differs from DIF bit-reversed in chunk {h}"
        ph("DIT = DIF bit-reversed")
        ph.report(ctx, buf.nbytes / 1e9)
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------------- computeH at 2^28
def test_compute_h_2p28_closed_form(ctx):
    ctx.trim()
    L = 28
    N = 1 << L
    ph = Phases("computeH 2^28")
    ta, tb = CF.compute_h_poly(L, seed=28)
    a, b, c, h = (ctx.alloc(32 * N) for _ in range(4))
    try:
        for dev, terms in ((a, ta), (b, tb)):
            for off, rows in CF.poly_eval_chunks(L, terms):
                _upload_at(ctx, dev, off, rows)
        ph("inputs")
        want = CF.compute_h_expected(L, ta, tb)
        ctx.field_op_dev(0, CF.MUL, c.ptr, a.ptr, b.ptr, N)
        for label, cp in (("c given", c.ptr), ("c = NULL", None)):
            ctx.compute_h_dev(L, a.ptr, b.ptr, cp, N, h.ptr)
            ctx.sync()
            ph(f"computeH {label}")
            got = h.download((N, 4))
            bad = CF.compute_h_check(got, L, ta, tb)
            del got
            ph("check")
            assert bad == [], f"computeH at 2^28, {label}: slots {bad[:8]} (expected {len(want)} non-zero coefficients)"
        ph.report(ctx, 4 * 32 * N / 1e9)
    finally:
        for d in (a, b, c, h):
            d.free()
