"""GPU suite: kSum of a whole batch over a window table of the key's K[1..] (include/mi355x_groth16_verify_ksum.h; csrc/ksum.hip over
ksum_ops.cuh).  Every coordinate is fully reduced, so a row's sum has one encoding: mi_vk_ksum_batch_dev must give, bit for bit, what
mi_msm_g1_dev gives for the row over the same bases -- the MSM the verifiers ran per proof before -- and, on a sample, the point
computed in the exponent (the bases are known multiples of the generator, tests/ksum_cases.py).  Every width is forced through the
budget; the tables stay below about 35 MB."""
import ctypes as C
import numpy as np
import pytest
import dlog_keys as D
import verify_cases as V
import verify_forge as F
import ksum_cases as K
from helpers import fr_arr
from gpu_common import load_binding

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 130)
NS_WIDTHS = [(ns, c) for ns in (1, 2, 5, 65, 300) for c in K.WIDTHS if c < 8 or ns <= 65]
N_MAX = max(SIZES)


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


def _affine(jac):
    """a normalised mi_g1_jac (Z = 1, or Z = 0 for infinity) -> the affine record, zeros for infinity"""
    jac = np.asarray(jac, np.uint64)
    return jac[:8].copy() if jac[8:].any() else np.zeros(8, np.uint64)


@pytest.fixture(scope="module")
def keys(ctx):
    """(ns, kind) -> the loaded key over known exponents, 130 rows of scalars on the device, and their sums by mi_msm_g1_dev row by
    row: computed once, shared by every test below and left unchanged"""
    made = {}
    shell = V.vk_arrays(F.forge_key(1, 0)["vk"])[0]

    def get(ns, kind="plain"):
        if (ns, kind) not in made:
            exps = K.key_exps(ns, kind)
            bases = ctx.batch_scalar_mul(D.G1, fr_arr(exps))
            assert bases.any(axis=1).tolist() == [e != 0 for e in exps]
            vkh = ctx.vk_load(dict(shell, k=np.concatenate([shell["k"][:1], bases])), ns + 1)
            rows = K.batch_rows(ns, N_MAX)
            scal = K.rows_arr(rows, ns)
            d_bases, d_scal = ctx.to_dev(bases), ctx.to_dev(scal)
            ref = np.stack([_affine(ctx.msm_g1_dev(d_bases.ptr, d_scal.ptr + 32 * ns * i, ns)) for i in range(N_MAX)])
            made[(ns, kind)] = dict(exps=exps, vkh=vkh, rows=rows, scal=scal, d_scal=d_scal, d_bases=d_bases, ref=ref)
        return made[(ns, kind)]
    yield get
    for k in made.values():
        k["vkh"].free(); k["d_scal"].free(); k["d_bases"].free()


def _prepare(k, ns, c):
    info = k["vkh"].ksum_prepare(K.budget_for(ns, c))
    B = load_binding()
    assert (info["window_bits"], info["windows"], info["table_bytes"], info["bases"], info["state"]) == (c, K.windows(c), K.table_bytes(ns, c), ns, B.KSUM_READY)
    assert info["table_bytes"] <= 36 << 20
    return info


def _sums_dev(ctx, k, ns, first, n, skip=None):
    out = ctx.alloc(64 * n)
    d_skip = None if skip is None else ctx.to_dev(np.ascontiguousarray(skip, np.uint8))
    try:
        out.upload(np.full((n, 8), 0x5555555555555555, np.uint64))
        k["vkh"].ksum_batch_dev(k["d_scal"].ptr + 32 * ns * first, None if d_skip is None else d_skip.ptr, n, out.ptr)
        ctx.sync()
        return out.download((n, 8))
    finally:
        out.free()
        if d_skip is not None:
            d_skip.free()


@pytest.mark.parametrize("ns,c", NS_WIDTHS)
def test_sums_equal_the_msm_row_by_row(ctx, keys, ns, c):
    """n in {1, 63, 64, 65, 130}: the edge rows first (all zero -> infinity, 1, r - 1, only the top window, byte values), one row alone
    is a full-width one; then the host-pointer call, and a sample against the exponent"""
    k = keys(ns)
    _prepare(k, ns, c)
    assert not k["ref"][0].any() and k["ref"][1:7].any(axis=1).all()
    for n in SIZES:
        first = 6 if n == 1 else 0
        got = _sums_dev(ctx, k, ns, first, n)
        want = k["ref"][first:first + n]
        assert np.array_equal(got, want), (ns, c, n, np.flatnonzero((got != want).any(axis=1))[:8])
    assert np.array_equal(k["vkh"].ksum_batch(k["scal"][:65]), k["ref"][:65])
    sample = [0, 1, 2, 3, 4, 5, 6, N_MAX - 1]
    assert np.array_equal(k["ref"][sample], K.expected_points(k["exps"], [k["rows"][i] for i in sample]))


@pytest.mark.parametrize("c", K.WIDTHS)
@pytest.mark.parametrize("ns,kind", [(1, "inf"), (2, "inf"), (5, "inf"), (2, "equal"), (5, "equal"), (2, "opposite"), (5, "opposite")])
def test_keys_with_infinite_equal_and_opposite_bases(ctx, keys, ns, kind, c):
    """a K[j] at infinity gives a row of infinities in the table; K[2] = K[1] with equal scalars is the doubling branch of the sum of a
    row's partials, with scalars that sum to r its cancellation; K[2] = -K[1] cancels on equal scalars"""
    k = keys(ns, kind)
    _prepare(k, ns, c)
    rows, ref = k["rows"], k["ref"]
    if ns > 1:
        assert rows[7][0] == rows[7][1] and (rows[8][0] + rows[8][1]) % K.r == 0
        if ns == 2:
            assert ref[7].any() != (kind == "opposite") and ref[8].any() != (kind == "equal")
    if ns == 1:
        assert not ref.any(), "the only base is infinity"
    for n in (1, 65, N_MAX):
        first = 7 if n == 1 and ns > 1 else 0
        assert np.array_equal(_sums_dev(ctx, k, ns, first, n), ref[first:first + n]), (ns, kind, c, n)
    assert np.array_equal(ref[:10], K.expected_points(k["exps"], rows[:10]))


def test_a_skipped_row_stays_infinity_whatever_its_words_are(ctx, keys):
    ns = 5
    k = keys(ns)
    _prepare(k, ns, 4)
    n = 65
    skip = np.zeros(n, np.uint8); skip[[0, 6, 7, 63, 64]] = 1
    junk = k["scal"][:n].copy(); junk[skip != 0] = np.uint64((1 << 64) - 1)      # words no field element has
    want = k["ref"][:n].copy(); want[skip != 0] = 0
    assert np.array_equal(k["vkh"].ksum_batch(junk, skip), want)
    assert np.array_equal(_sums_dev(ctx, k, ns, 0, n, skip), want)
    assert not k["vkh"].ksum_batch(junk, np.ones(n, np.uint8)).any()


def test_a_rebuild_at_another_budget_gives_the_same_points(ctx, keys):
    ns = 5
    k = keys(ns)
    seen = []
    for c in (8, 2, 4, 8):
        info = _prepare(k, ns, c)
        assert info["budget_bytes"] == K.budget_for(ns, c) and info["build_ms"] > 0
        assert k["vkh"].ksum_prepare(K.budget_for(ns, c))["build_ms"] == info["build_ms"], "the same budget again is no work"
        seen.append(_sums_dev(ctx, k, ns, 0, N_MAX))
    assert all(np.array_equal(s, k["ref"]) for s in seen)


def test_a_batch_whose_lanes_exceed_one_capped_grid(ctx, keys):
    """260 rows of 65 scalars at c = 4: 1009 slices per row, 262340 lanes against a grid of 4096 workgroups of 64 -- the first lanes of
    the grid take a second item; the reference rows are the 130 of the fixture, twice"""
    ns, c, n = 65, 4, 260
    k = keys(ns)
    _prepare(k, ns, c)
    assert K.slices(ns, c, n) * n > K.GRID_CAP_LANES >= K.slices(ns, c, N_MAX) * N_MAX
    scal = np.concatenate([k["scal"], k["scal"][::-1]])
    want = np.concatenate([k["ref"], k["ref"][::-1]])
    assert np.array_equal(k["vkh"].ksum_batch(scal), want)


def test_budget_info_and_refusals(ctx, keys):
    """a budget below the narrowest table: no table, and the info says so; the argument errors are decided on the host and name the
    argument; a key without bases has nothing to sum"""
    B = load_binding()
    ns = 2
    k = keys(ns)
    vkh, lib = k["vkh"], ctx.lib
    info = vkh.ksum_prepare(K.table_bytes(ns, 2) - 1)
    assert (info["window_bits"], info["windows"], info["table_bytes"], info["state"]) == (0, 0, 0, B.KSUM_OVER_BUDGET)
    out = np.full((2, 8), 7, np.uint64)
    sc = k["scal"][:2]

    def refused(message, vk, scalars, n, o, dev=False):
        f = lib.mi_vk_ksum_batch_dev if dev else lib.mi_vk_ksum_batch
        assert f(ctx.h, vk, scalars, None, C.c_size_t(n), o) == -1, message
        assert lib.mi_last_error(ctx.h).decode().startswith(f"ksum: {message}"), lib.mi_last_error(ctx.h)
        assert (out == 7).all()

    refused("the key has no table", vkh.h, V.p_(sc), 2, V.p_(out))
    assert vkh.ksum_prepare(0)["window_bits"] == 8 and vkh.ksum_info()["budget_bytes"] == B.KSUM_DEFAULT_TABLE_BYTES
    for dev in (False, True):
        refused("vk is null", None, V.p_(sc), 2, V.p_(out), dev)
        refused("scalars is null", vkh.h, None, 2, V.p_(out), dev)
        refused("out is null", vkh.h, V.p_(sc), 2, None, dev)
        refused("n is above 2^24", vkh.h, V.p_(sc), (1 << 24) + 1, V.p_(out), dev)
    assert lib.mi_vk_ksum_batch(ctx.h, vkh.h, None, None, C.c_size_t(0), None) == 0
    assert lib.mi_vk_ksum_prepare(ctx.h, None, C.c_uint64(0)) == -1 and lib.mi_last_error(ctx.h).decode() == "ksum: vk is null"
    assert lib.mi_vk_ksum_get_info(ctx.h, vkh.h, None) == -1 and lib.mi_last_error(ctx.h).decode() == "ksum: the info pointer is null"
    # K[0] alone
    d, nbp, ped = V.vk_arrays(F.forge_key(1, 0)["vk"])
    bare = ctx.vk_load(d, nbp, ped)
    try:
        info = bare.ksum_prepare(0)
        assert (info["window_bits"], info["bases"], info["state"]) == (0, 0, B.KSUM_NO_BASES)
        refused("the key has no bases", bare.h, V.p_(sc), 1, V.p_(out))
        assert lib.mi_vk_ksum_batch(ctx.h, bare.h, None, None, C.c_size_t(0), None) == 0
    finally:
        bare.free()
