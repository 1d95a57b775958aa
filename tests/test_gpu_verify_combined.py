"""GPU suite: one verdict for a batch of proofs (include/mi355x_groth16_verify_combined.h) -- the two new kernels through their debug entry
points against the host build of the same text (tests/emu/emu_verify_combined.cpp), every batch of tests/test_verify_combined_cpu.py
against the host build and the verdict in the exponent (tests/verify_combine_ref.py), real Setup / Prove proofs with one tamper per
verdict, the library's own seed, the bytes twin, consistency with mi_groth16_verify_batch, and the refusals."""
import ctypes as C
import numpy as np
import pytest
import pyref as P
import cref
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import verify_combine_ref as CR
import verify_combined_cases as VC
import bytes_cases as BC
import setup_cases as S
import r1cs_cases as RC
import dlog_keys as D
from helpers import fr_arr, fr_vals, g1_arr, g1_pts
from gpu_common import load_binding

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
    return C.CDLL(VC.build_emu(str(tmp_path_factory.mktemp("emu") / "libemu_verify_combined.so")))


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


# ---------------------------------------------------------------------------------------------------- the two kernels alone
@pytest.mark.parametrize("n", [1, 2, 9, 63, 64, 65, 129, 130])
def test_fp12_product_equals_the_host_build_word_for_word(ctx, emu, n):
    """fan-in 8: 9 and 65 leave a lone value at their first level, 130 -> 17 -> 3 -> 1 leaves one at its second; 65, 129 and 130 take
    three levels; the sequential product of the host build groups the factors differently and must give the same words"""
    rng = np.random.default_rng(900 + n)
    xs = [[int.from_bytes(rng.bytes(31), "little") for _ in range(12)] for _ in range(n)]
    X = V.gt_arr(xs)
    assert np.array_equal(ctx.fp12_product(X), VC.emu_product(emu, X))
    X1 = X.copy(); X1[0] = V.gt_arr([R.to_tower(R.ONE)])[0]
    got = ctx.fp12_product(X1)
    assert np.array_equal(got, VC.emu_product(emu, X1))
    if n == 1:
        assert np.array_equal(got, X1[0])
    if n == 2:
        assert V.gt_vals(ctx.fp12_product(X)) == [R.to_tower(R.f_mul(R.from_tower(xs[0]), R.from_tower(xs[1])))]


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_g1_scale128_equals_the_host_build(ctx, emu, n):
    rng = np.random.default_rng(950 + n)
    pts = V.seeded_pairs(n, 960 + n, inf_first_last=False)[0]
    ks = ([M128, 0, 1, 2, 1 << 127, 1 << 64] + [int.from_bytes(rng.bytes(16), "little") for _ in range(n)])[:n]
    if n > 1:
        pts[5] = None                                   # infinity under a random coefficient
        assert ks[5] == 1 << 64
        pts[n - 1] = None
    pa = g1_arr(pts)
    got = ctx.g1_scale128(pa, ks)
    assert np.array_equal(got, VC.emu_scale128(emu, pa, ks))
    for i in sorted({0, 1, 5, n - 2, n - 1} & set(range(n))):
        assert g1_pts(got[i:i + 1])[0] == (P.g1_mul(pts[i], ks[i]) if pts[i] is not None and ks[i] else None), i


# ---------------------------------------------------------------------------------------------------- the batches of the CPU suite
def _check(emu, vkh, batch):
    """the device's verdict and index against the host build's and the exponent's; then against the per-proof verifier"""
    key, cases, seed = batch["key"], batch["cases"], batch["seed"]
    inputs = [F.verify_input(c) for c in cases]
    want = CR.combined_verdict_in_exponent(key, cases, seed)
    assert want == batch["want"], batch["name"]
    got = vkh.verify_combined(inputs, seed)
    assert got == want == VC.emu_verify_combined(emu, key["vk"], inputs, seed), batch["name"]
    each = list(vkh.verify_batch(inputs))
    assert each == [F.verdict_in_exponent(key, c) for c in cases], batch["name"]
    if not batch["crafted_for_seed"]:
        assert (got[0] == R.OK) == (not any(each)), batch["name"]
    assert (got[0] == R.MALFORMED) == (R.MALFORMED in each), batch["name"]
    if got[0] == R.MALFORMED:
        assert got[1] == each.index(R.MALFORMED), batch["name"]


@pytest.mark.parametrize("group", ["accepted_batches", "single_batches", "cancelling_batches", "distinct_batches"])
def test_every_batch_of_the_cpu_suite(emu, forged_vk, group):
    for batch in getattr(CR, group)():
        _check(emu, forged_vk(batch["key"]), batch)


def test_a_batch_of_130_then_small_ones_in_its_workspace(emu, forged_vk):
    """three waves of Miller loops with a partial last one, four levels of the product (133 -> 17 -> 3 -> 1)"""
    key = F.forge_key(3, 1)
    vkh = forged_vk(key)
    cases = [dict(F.honest(key, 1300 + i), name=f"entry {i}") for i in range(130)]
    _check(emu, vkh, {"name": "130 honest", "key": key, "cases": cases, "seed": CR.SEED_B, "want": (R.OK, 130), "crafted_for_seed": False})
    bad = list(cases); bad[129] = CR.shift_groth(key, cases[129], 1)
    _check(emu, vkh, {"name": "130, Krs of the last off by one", "key": key, "cases": bad, "seed": CR.SEED_A, "want": (R.PAIRING, 130), "crafted_for_seed": False})
    for n, want in ((1, R.PAIRING), (3, R.PAIRING)):
        _check(emu, vkh, {"name": f"the last {n}", "key": key, "cases": bad[130 - n:], "seed": CR.SEED_A, "want": (want, n), "crafted_for_seed": False})
    _check(emu, vkh, {"name": "the first 3", "key": key, "cases": bad[:3], "seed": CR.SEED_A, "want": (R.OK, 3), "crafted_for_seed": False})


def test_a_batch_of_130_with_three_commitments(emu, forged_vk):
    """three blocks per column of the column-sum kernel, the last one partial, with fold challenges: the blocks of column S write
    r_i c_i^k for k = 0, 1, 2 across all three (the larger batches above have one commitment, where that product is r_i alone); a
    Pedersen defect of the last proof, in the partial block, is seen"""
    key = F.forge_key(3, 3)
    vkh = forged_vk(key)
    cases = [dict(F.honest(key, 1300 + i), name=f"entry {i}") for i in range(130)]
    _check(emu, vkh, {"name": "130 honest, 3 commitments", "key": key, "cases": cases, "seed": CR.SEED_B, "want": (R.OK, 130), "crafted_for_seed": False})
    bad = list(cases); bad[129] = CR.shift_pedersen(cases[129], 1)
    _check(emu, vkh, {"name": "130, pok of the last off by one", "key": key, "cases": bad, "seed": CR.SEED_A, "want": (R.PEDERSEN, 130), "crafted_for_seed": False})


# ---------------------------------------------------------------------------------------------------- real proofs
@pytest.fixture(scope="module", params=[0, 2])
def made(ctx, request):
    """a solvable skewed R1CS of 600 constraints, its key by mi_groth16_setup under a random trapdoor, its proof by mi_groth16_prove_w or
    mi_prover_submit_bsb22 -- the recipe of tests/test_gpu_verify_bytes.py::made: the value of commitment wire i IS the hash of commitment
    i, so the same proof passes the struct entry point and, written out by mi_proof_write, the bytes one"""
    B = load_binding()
    nc = request.param
    n, nab, nb_public = 600, 300, 5
    r1cs = RC.skewed_r1cs(n, nab, nb_public, 140 + nc, long_lens=(16, 17, 64), commitments=nc, n_committed=7)
    r1cs["commitments"] = sorted(r1cs["commitments"], key=lambda c: c[1])
    r1cs["nb_wires"] = nab + n
    r1cs["C"] = (np.arange(n + 1, dtype=np.uint64), (nab + np.arange(n)).astype(np.uint32), np.ones(n, np.uint32))
    W = np.zeros((r1cs["nb_wires"], 4), np.uint64)
    W[:nab] = RC.witness(nab, 141 + nc)
    td = S.synth_trapdoor(150 + nc, n_sigma=nc)
    rr, ss = cref.gen_scalars(2, 160 + nc, 0)
    pkh, peds, vk = ctx.setup(r1cs, td)
    pub = fr_vals(W[1:nb_public])
    pool = B.Prover(0, 1) if nc else None
    try:
        vals = [np.ascontiguousarray(W[ws]) for ws, _ in r1cs["commitments"]]
        cms = np.stack([pool.commit(peds[k], vals[k]).reshape(8) for k in range(nc)]) if nc else np.zeros((0, 8), np.uint64)
        values, fold = BC.bsb22_hashes(g1_pts(cms), pub)
        for (_, cw), v in zip(r1cs["commitments"], values):
            W[cw] = fr_arr([v])[0]
        a, b = RC.eval_rows(r1cs, "A", W), RC.eval_rows(r1cs, "B", W)
        W[nab:] = D._op(2, a, b)
        if nc:
            proof, _ = pool.wait(pool.submit_bsb22(pkh, W, a, b, None, rr, ss, [(peds[k], vals[k]) for k in range(nc)], fr_arr([fold])[0]))
        else:
            rh = ctx.r1cs_load(r1cs)
            proof, _ = ctx.prove_w(pkh, rh, W, rr, ss)
            ctx.r1cs_free(rh)
    finally:
        if pool:
            pool.close()
    inp = {"raw": proof["raw"].copy(), "public_inputs": np.ascontiguousarray(W[1:nb_public])}
    ped_vk = None
    if nc:
        ped_vk = ctx.pedersen_vk_make(np.stack(td["sigma"]))
        inp.update(commitments=cms, pok=np.ascontiguousarray(proof["pok"]).reshape(8), fold_challenge=fr_arr([fold])[0], commitment_values=fr_arr(values))
    vkh = ctx.vk_load(vk, nb_public, ped_vk)
    yield dict(nc=nc, vkh=vkh, inp=inp, cms=cms)
    vkh.free()
    for pd in peds:
        ctx.pedersen_pk_free(pd)
    ctx.pk_free(pkh)


def _other_g1(k):
    return g1_arr([P.g1_mul(P.G1_GEN, 1000 + k)])[0]


def _tampered(made):
    """[(name, proof, the verdict it gets alone)]"""
    inp = made["inp"]
    x = inp["raw"].copy(); x[24:32] = _other_g1(2)
    out = [("Krs", dict(inp, raw=x), R.PAIRING)]
    if made["nc"]:
        out.append(("pok", dict(inp, pok=_other_g1(3)), R.PEDERSEN))
    return out


def _consistent(vkh, proofs, got):
    each = list(vkh.verify_batch(proofs))
    assert (got[0] == R.OK) == (not any(each))
    assert (got[0] == R.MALFORMED) == (R.MALFORMED in each) and (got[0] != R.MALFORMED or got[1] == each.index(R.MALFORMED))


def test_real_proofs_one_tamper_per_verdict(made):
    vkh, inp = made["vkh"], made["inp"]
    for seed in (CR.SEED_A, None):           # None: the library draws the seed; a wrong accept has probability about 2^-128 (the scheme's)
        got = vkh.verify_combined([inp] * 3, seed)
        assert got == (R.OK, 3)
        _consistent(vkh, [inp] * 3, got)
        for name, bad, want in _tampered(made):
            for at in (0, 2):
                proofs = [inp] * 3; proofs[at] = bad
                got = vkh.verify_combined(proofs, seed)
                assert got == (want, 3), (name, at, seed)
                _consistent(vkh, proofs, got)
    assert vkh.verify_combined([inp], None) == (R.OK, 1)
    y = inp["raw"].copy(); y[0:8] = g1_arr([(1, 3)])[0]
    proofs = [inp, _tampered(made)[0][1], dict(inp, raw=y), dict(inp, raw=y)]
    got = vkh.verify_combined(proofs)
    assert got == (R.MALFORMED, 2)
    _consistent(vkh, proofs, got)


def test_bytes_twin(made):
    B = load_binding()
    vkh, inp, nc = made["vkh"], made["inp"], made["nc"]
    data = B.proof_write(inp["raw"], commitments=made["cms"] if nc else None, pok=inp.get("pok"))
    pub = inp["public_inputs"]
    for seed in (CR.SEED_A, None):
        assert vkh.verify_bytes_combined([(data, pub)] * 3, seed) == (R.OK, 3)
    assert list(vkh.verify_bytes_batch([(data, pub)] * 3)) == [R.OK] * 3
    p_bytes = R.p.to_bytes(32, "big")
    assert p_bytes[0] < 0x40
    not_below_p = bytes([0x80 | p_bytes[0]]) + p_bytes[1:] + data[32:]       # Ar: the flag of a compressed point, X = p
    for i in (0, 2):
        items = [(data, pub)] * 3; items[i] = (not_below_p, pub)
        assert vkh.verify_bytes_combined(items, CR.SEED_A) == (R.MALFORMED, i)
        assert list(vkh.verify_bytes_batch(items)).index(R.MALFORMED) == i
    other = pub.copy(); other[0] = fr_arr([D._int(other[0]) + 1])[0]
    assert vkh.verify_bytes_combined([(data, pub), (data, other)], None) == (R.PAIRING, 2)
    assert vkh.verify_bytes_combined([], None) == (R.OK, 0)
    with pytest.raises(B.MiError, match="proof_len"):
        vkh.verify_bytes_combined([(data[:-1], pub)], None)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx, made):
    B = load_binding()
    lib, vkh, inp = ctx.lib, made["vkh"], made["inp"]
    arr, keep = vkh._inputs([inp])
    v, first = C.c_uint8(255), C.c_uint64(77)
    call = lambda vk, a, n, vd: lib.mi_groth16_verify_combined(ctx.h, vk, a, C.c_size_t(n), CR.SEED_A, vd, C.byref(first))
    assert call(None, arr, 1, C.byref(v)) == -1 and call(vkh.h, None, 1, C.byref(v)) == -1 and call(vkh.h, arr, 1, None) == -1
    assert call(vkh.h, arr, (1 << 24) + 1, C.byref(v)) == -1
    assert call(vkh.h, None, 0, None) == -1                     # the ONE verdict is written for an empty batch too
    assert (v.value, first.value) == (255, 77)                  # a refusal writes nothing
    with pytest.raises(B.MiError, match="public_inputs is null"):
        vkh.verify_combined([{k: x for k, x in inp.items() if k != "public_inputs"}], CR.SEED_A)
    if made["nc"]:
        for name in ("commitments", "pok", "commitment_values", "fold_challenge"):
            with pytest.raises(B.MiError, match="is null"):
                vkh.verify_combined([inp, {k: x for k, x in inp.items() if k != name}], CR.SEED_A)
    assert call(vkh.h, None, 0, C.byref(v)) == 0 and (v.value, first.value) == (R.OK, 0)
    assert vkh.verify_combined([], None) == (R.OK, 0)
    assert vkh.verify_combined([inp], CR.SEED_A) == (R.OK, 1)
