"""GPU suite: one verdict per proof at the combined test's price (include/mi355x_groth16_verify_locate.h) -- the three new kernels through
their debug entry points against the host build of the same text (tests/emu/emu_verify_locate.cpp), the batches of
tests/test_verify_locate_cpu.py against the host build, the exponent (tests/verify_locate_ref.py) and the device's own per-proof
verifier, real Setup / Prove proofs, the library's own seed, the bytes twin, the reuse of the workspace, and the refusals."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import verify_combine_ref as CR
import verify_locate_ref as LR
import verify_locate_cases as LC
from helpers import fr_arr, g1_arr, g1_pts
from gpu_common import load_binding
from test_gpu_verify_combined import made, _tampered      # the recipe of real proofs (a module-scoped fixture) and its tampers

pytestmark = pytest.mark.gpu
M128 = (1 << 128) - 1


@pytest.fixture(scope="module")
def ctx():
    B = load_binding()
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.CDLL(LC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_locate.so")))


@pytest.fixture(scope="module")
def forged_vk(ctx):
    loaded = {}

    def get(key):
        if key["id"] not in loaded:
            d, nbp, ped = V.vk_arrays(key["vk"])
            loaded[key["id"]] = ctx.vk_load(d, nbp, ped)
        return loaded[key["id"]]
    yield get
    for h in loaded.values():
        h.free()


# ---------------------------------------------------------------------------------------------------- the new kernels alone
@pytest.mark.parametrize("n", [1, 8, 9, 65, 130])
def test_g1_sum_tree_equals_the_host_build_word_for_word(ctx, emu, n):
    """infinities at 0, 5 and n - 1; one run of 8 holds A, -A (the accumulator cancels to infinity) and then B, B (it doubles)"""
    pts = V.seeded_pairs(n, 2100 + n, inf_first_last=False)[0]
    for i in {0, 5, n - 1} & set(range(n)):
        pts[i] = None
    at = 8 if n > 16 else 1
    if n >= 8:
        pts[at + 1] = P.g1_neg(pts[at])
        pts[at + 3] = pts[at + 2]
    pa = g1_arr(pts)
    got = ctx.g1_sum_tree(pa)
    assert np.array_equal(got, LC.emu_sum_tree(emu, pa))
    total = None
    for q in pts:
        total = P.g1_add(total, q)
    assert g1_pts(got[-1:])[0] == total                            # the root is the sum of all
    cnt = LR.level_counts(n)
    assert len(got) == sum(cnt[1:])
    assert g1_pts(got[:1])[0] == _sum(pts[:8])


def _sum(pts):
    acc = None
    for q in pts:
        acc = P.g1_add(acc, q)
    return acc


@pytest.mark.parametrize("nc", [0, 1, 3])
def test_locate_points_equal_the_host_build(ctx, emu, nc):
    n = 67
    rng = np.random.default_rng(2200 + nc)
    mk = lambda seed: g1_arr(V.seeded_pairs(n, seed, inf_first_last=False)[0])
    krs, pok = mk(2210 + nc), mk(2220 + nc)
    cm = np.stack([mk(2230 + 10 * nc + k) for k in range(nc)], axis=1) if nc else None
    fold = fr_arr([0, 1, 2, R.r - 1] + [int.from_bytes(rng.bytes(31), "little") for _ in range(n - 4)]) if nc > 1 else None
    rs = [0, 1, M128, 1 << 127] + [int.from_bytes(rng.bytes(16), "little") for _ in range(n - 4)]       # k = 0 gives infinities
    krs[5] = 0; pok[6] = 0                                                                              # infinite inputs
    if nc:
        cm[7] = 0
        cm[8, 0] = 0
    got = ctx.locate_points(rs, krs, cm, pok if nc else None, fold)
    want = LC.emu_points(emu, rs, krs, cm, pok if nc else None, fold)
    assert got.shape == want.shape == (1 + (2 if nc else 0) + (nc if nc > 1 else 0), n, 8)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2)).tolist()       # (array, proof) that differ
    assert not got[:, 0].any() and not got[0, 5].any()
    assert g1_pts(got[0, 2:3])[0] == P.g1_mul(g1_pts(krs[2:3])[0], M128)
    if nc:
        assert g1_pts(got[1, 9:10])[0] == P.g1_mul(_sum(g1_pts(cm[9])), rs[9]) and not got[2, 6].any() and not got[1, 7].any()
    if nc > 1:
        assert np.array_equal(got[3, 1], cm[1, 0]) and np.array_equal(got[4, 1], cm[1, 1])     # r = 1, c = 1: the commitments themselves
        assert g1_pts(got[3, 2:3])[0] == P.g1_mul(g1_pts(cm[2, :1])[0], M128)                  # c^0 = 1 whatever c is
        assert not got[4, 0].any() and g1_pts(got[4, 3:4])[0] == P.g1_mul(g1_pts(cm[3, 1:2])[0], (1 << 127) * (R.r - 1) % R.r)


@pytest.mark.parametrize("ns", [0, 1, 5])
def test_segmented_column_sums_equal_the_host_build(ctx, emu, ns):
    """130 rows: the last node of level 1 has two of them, the last of level 2 has two as well (128, 129), the root all; 600 rows at the
    root run more than one block per node"""
    for n, queries in ((130, [(1, [0, 3, 16]), (1, list(range(17))), (2, [2, 0]), (3, [0]), (0, [129, 0, 64])]), (600, [(4, [0]), (3, [1, 0]), (2, [9, 4])])):
        rng = np.random.default_rng(2300 + ns + n)
        rs = [0, M128] + [int.from_bytes(rng.bytes(16), "little") for _ in range(n - 2)]
        vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(ns)] for _ in range(n)]
        scal = np.stack([fr_arr(v) for v in vals]) if ns else np.zeros((n, 0, 4), np.uint64)
        for level, nodes in queries:
            got = ctx.locate_colsums(scal, rs, level, nodes)
            assert np.array_equal(got, LC.emu_colsums(emu, scal, rs, level, nodes)), (n, level)
            for t, j in enumerate(nodes):
                rows = LR.node_range(n, level, j)
                want = [sum(rs[i] * vals[i][c] for i in rows) % R.r for c in range(ns)] + [sum(rs[i] for i in rows) % R.r]
                assert np.array_equal(got[t], fr_arr(want)), (n, level, j)


# ---------------------------------------------------------------------------------------------------- the batches of the CPU suite
def _check(ctx, emu, vkh, name, key, cases, inputs, seed, cap=None, crafted=False):
    """the device against the model in the exponent, the host build and (unless crafted for its seed) the device's per-proof verifier"""
    want, want_stats = LR.model(key, cases, seed, cap)
    ctx.set_locate_round_nodes(cap or 0)
    try:
        got, stats = vkh.verify_locate(inputs, seed)
    finally:
        ctx.set_locate_round_nodes(0)
    assert list(got) == want, (name, cap)
    assert stats == want_stats, (name, cap, stats, want_stats)
    assert (list(got), stats) == LC.emu_verify_locate(emu, key["vk"], inputs, seed, cap), (name, cap)
    if not crafted:
        assert list(got) == LR.expected_each(key, cases) == list(vkh.verify_batch(inputs)), (name, cap)
    return list(got), stats


@pytest.mark.parametrize("cap", LC.CAPS)
@pytest.mark.parametrize("which", LC.BAD_POSITION_NAMES)
def test_bad_positions_of_130(ctx, emu, forged_vk, which, cap):
    name, key, cases, inputs = LC.bad_position_cases()[which]
    got, stats = _check(ctx, emu, forged_vk(key), name, key, cases, inputs, CR.SEED_A, cap)
    if cap is None and which == "a":
        assert stats["judged_alone"] == 8 and stats["nodes_tested"] == 18
    if cap is None and which == "b":
        assert stats["judged_alone"] == 2


def test_precedence_of_the_verdicts(ctx, emu, forged_vk):
    key, cases = LC.precedence_batch()
    got, _ = _check(ctx, emu, forged_vk(key), "precedence", key, cases, [F.verify_input(c) for c in cases], CR.SEED_A)
    assert got[2] == R.PAIRING and got[7] == R.PEDERSEN


@pytest.mark.parametrize("shape", [(3, 1), (3, 3)])
def test_malformed_proofs_do_not_end_the_batch(ctx, emu, forged_vk, shape):
    key = F.forge_key(*shape)
    cases = F.distinct_batch(key, 70, 700 + shape[1])
    got, stats = _check(ctx, emu, forged_vk(key), "70 distinct", key, cases, [F.verify_input(c) for c in cases], CR.SEED_A, 1 if shape[1] == 1 else None)
    assert [i for i, v in enumerate(got) if v == R.MALFORMED] == [0, 63, 69] and stats["malformed"] == 3 and stats["rejected"] == 2


def test_nodes_reuse_the_coefficients_of_the_batch(ctx, emu, forged_vk):
    for name, key, cases, seed, crafted in LC.crafted_batches():
        got, stats = _check(ctx, emu, forged_vk(key), name, key, cases, [F.verify_input(c) for c in cases], seed, None, crafted)
        if crafted and len(cases) == 20:
            assert [got[3], got[5], got[17]] == [R.OK, R.OK, R.PAIRING]
        if crafted and len(cases) == 2:
            assert got == [R.OK, R.OK] and stats["rounds"] == 1


def test_a_batch_of_130_then_small_ones_in_its_workspace(ctx, emu, forged_vk):
    """the layouts of the three bodies do not leak into each other: 130, then 1 and 3 on the same context, then the other two calls"""
    key, base = LC.honest_130()
    ins = list(LC.inputs_130())
    vkh = forged_vk(key)
    cases = list(base); cases[129] = CR.shift_groth(key, base[129], 1)
    bad = list(ins); bad[129] = F.verify_input(cases[129])
    _check(ctx, emu, vkh, "130 honest", key, list(base), ins, CR.SEED_B)
    _check(ctx, emu, vkh, "130, the last off by one", key, cases, bad, CR.SEED_A)
    for n in (1, 3):
        got, stats = _check(ctx, emu, vkh, f"the last {n}", key, cases[130 - n:], bad[130 - n:], CR.SEED_A)
        assert got == [R.OK] * (n - 1) + [R.PAIRING] and stats["judged_alone"] == n
    assert vkh.verify_combined(bad, CR.SEED_A) == (R.PAIRING, 130) and vkh.verify_combined(ins[:3], CR.SEED_A) == (R.OK, 3)
    assert list(vkh.verify_batch(bad[120:])) == [R.OK] * 9 + [R.PAIRING]
    got, _ = vkh.verify_locate(bad, CR.SEED_B)
    assert list(got) == [R.OK] * 129 + [R.PAIRING]


# ---------------------------------------------------------------------------------------------------- real proofs
def test_real_proofs_and_the_bytes_twin(made):
    B = load_binding()
    vkh, inp, nc = made["vkh"], made["inp"], made["nc"]
    tampers = {name: bad for name, bad, _ in _tampered(made)}
    proofs = [inp] * 9
    proofs[8] = tampers["Krs"]
    want = [R.OK] * 8 + [R.PAIRING]
    if nc:
        proofs[0] = tampers["pok"]
        want[0] = R.PEDERSEN
    for seed in (CR.SEED_A, None):            # None: the library draws the seed
        got, stats = vkh.verify_locate(proofs, seed)
        assert list(got) == want == list(vkh.verify_batch(proofs)), seed
        assert stats["rejected"] == (2 if nc else 1) and stats["malformed"] == 0 and stats["rounds"] >= 1
        got, stats = vkh.verify_locate([inp] * 9, seed)
        assert list(got) == [R.OK] * 9 and stats == {"rounds": 1, "nodes_tested": 1, "judged_alone": 0, "malformed": 0, "rejected": 0}
    # ---- the bytes twin on the same nine
    write = lambda pr: B.proof_write(pr["raw"], commitments=made["cms"] if nc else None, pok=pr.get("pok"))
    pub = inp["public_inputs"]
    items = [(write(pr), pub) for pr in proofs]
    for seed in (CR.SEED_A, None):
        got, stats = vkh.verify_bytes_locate(items, seed)
        assert list(got) == want and stats["rejected"] == (2 if nc else 1)
    data = items[1][0]
    p_bytes = R.p.to_bytes(32, "big")
    items[2] = (bytes([0x80 | p_bytes[0]]) + p_bytes[1:] + data[32:], pub)          # Ar does not decode: X = p
    got, stats = vkh.verify_bytes_locate(items, CR.SEED_A)
    assert list(got) == want[:2] + [R.MALFORMED] + want[3:] and stats["malformed"] == 1
    assert list(got) == list(vkh.verify_bytes_batch(items))
    got, stats = vkh.verify_bytes_locate([], None)
    assert len(got) == 0 and not any(stats.values())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(ctx, made):
    B = load_binding()
    lib, vkh, inp = ctx.lib, made["vkh"], made["inp"]
    arr, keep = vkh._inputs([inp, inp])
    v, st = (C.c_uint8 * 2)(9, 9), B.VerifyLocateStats(7, 7, 7, 7, 7)
    call = lambda c, vk, a, n, vd: lib.mi_groth16_verify_locate(c, vk, a, C.c_size_t(n), CR.SEED_A, vd, C.byref(st))
    assert call(None, vkh.h, arr, 2, v) == -1 and call(ctx.h, None, arr, 2, v) == -1 and call(ctx.h, vkh.h, None, 2, v) == -1
    assert call(ctx.h, vkh.h, arr, 2, None) == -1 and call(ctx.h, vkh.h, arr, (1 << 24) + 1, v) == -1
    untouched = lambda: list(v) == [9, 9] and set(st.as_dict().values()) == {7}
    assert untouched()
    with pytest.raises(B.MiError, match="public_inputs is null"):
        vkh.verify_locate([inp, {k: x for k, x in inp.items() if k != "public_inputs"}], CR.SEED_A)
    bad, _keep = vkh._inputs([inp, {k: x for k, x in inp.items() if k != "public_inputs"}])
    assert call(ctx.h, vkh.h, bad, 2, v) == -1 and untouched()
    if made["nc"]:
        for name in ("commitments", "pok", "commitment_values", "fold_challenge"):
            bad, _keep = vkh._inputs([inp, {k: x for k, x in inp.items() if k != name}])
            assert call(ctx.h, vkh.h, bad, 2, v) == -1 and untouched(), name
    assert call(ctx.h, vkh.h, None, 0, None) == 0 and list(v) == [9, 9] and not any(st.as_dict().values())     # an empty batch: zeroed stats
    assert call(ctx.h, vkh.h, arr, 2, v) == 0 and list(v) == [R.OK, R.OK] and st.as_dict()["nodes_tested"] == 1
