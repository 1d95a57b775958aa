"""The combined batch verifier (include/mi355x_groth16_verify_combined.h) in the exponent, for tests/test_verify_combined_cpu.py and
tests/test_gpu_verify_combined.py.  Built on tests/verify_forge.py; nothing here calls the code under test.

With every discrete log of the key known, the two combined equations are sums of the per-proof defects
    d_i = a_i b_i - (alpha beta + ksum_i gamma + krs_i delta)          e_i = pok_i - sum_k sigma_k c_i^k m_ik
weighted by the coefficients: sum r_i d_i = 0 (else 1), then sum r_i e_i = 0 (else 2).  Verdict 3 comes from a case's structure, as in
verify_forge.verdict_in_exponent, and carries the lowest such index."""
import hashlib
import pairing_ref as R
import verify_forge as F

r = F.r
TAG = b"mi355x-g16-combine"
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


def coefficients(seed, n):
    """r_i = the little-endian integer of the first 16 bytes of SHA-256(TAG | seed | le64(n) | le64(i))"""
    assert len(seed) == 32
    return [int.from_bytes(hashlib.sha256(TAG + seed + n.to_bytes(8, "little") + i.to_bytes(8, "little")).digest()[:16], "little")
            for i in range(n)]


def groth_defect(key, case):
    e = key["exps"]
    rhs = e["alpha"] * e["beta"] + F.ksum_e(key, case["pub"], case["cv"], case["cm"]) * e["gamma"] + case["krs"] * e["delta"]
    return (case["a"] * case["b"] - rhs) % r


def pedersen_defect(key, case):
    return (case["pok"] - F.pok_of(key, case["cm"], case["fold"])) % r if key["n_commitments"] else 0


def combined_verdict_in_exponent(key, cases, seed):
    """(verdict, first_malformed): (3, lowest index) if any case is malformed or carries words; else 1, 2 or 0 with n"""
    n = len(cases)
    for i, c in enumerate(cases):
        if c["malformed"] or c["words"]:
            return R.MALFORMED, i
        assert not c["points"], "a named point without a reason why it is malformed"
    rs = coefficients(seed, n)
    if sum(ri * groth_defect(key, c) for ri, c in zip(rs, cases)) % r:
        return R.PAIRING, n
    if sum(ri * pedersen_defect(key, c) for ri, c in zip(rs, cases)) % r:
        return R.PEDERSEN, n
    return R.OK, n


def shift_groth(key, case, t):
    """the case with its Groth16 defect moved by t: krs - t / delta"""
    return F.but(case, krs=(case["krs"] - t * F.inv(key["exps"]["delta"])) % r)


def shift_pedersen(case, t):
    """the case with its Pedersen defect moved by t: pok + t"""
    return F.but(case, pok=(case["pok"] + t) % r)


# ---------------------------------------------------------------------------------------------------- the batches both suites run
T = 0x1F2E3D4C5B6A79881726354453627180


def _batch(name, key, cases, seed, want, crafted_for_seed=False):
    """crafted_for_seed: the defects were chosen KNOWING the coefficients of this seed -- the one way to make the combined verdict differ
    from the per-proof ones, and why the header asks for a seed the maker of the proofs cannot predict"""
    return {"name": f"{key['id']}: {name}", "key": key, "cases": list(cases), "seed": seed, "want": want, "crafted_for_seed": crafted_for_seed}


def accepted_batches():
    """per key of verify_forge.cases(): every accepted case as ONE batch (infinite K, Krs, C_k and pok, kSum at infinity, both group-law
    branches, every fold power)"""
    out = []
    for key in F.keys_of(F.cases()):
        mine = [c for c in F.cases() if c["key"]["id"] == key["id"] and c["want"] == R.OK]
        out.append(_batch("every accepted case", key, mine, SEED_A, (R.OK, len(mine))))
    return out


def single_batches():
    return [_batch(f"alone: {c['name']}", c["key"], [c], SEED_B, (R.OK, 1)) for c in F.cases() if c["want"] == R.OK]


def cancelling_batches():
    """two proofs whose defects are +t and -t (an unweighted sum passes), and two whose defects are r_1 t and -r_0 t under SEED_A (the
    weighted sum passes under SEED_A alone)"""
    out = []
    r0, r1 = coefficients(SEED_A, 2)
    for shape in ((2, 0), (3, 1), (3, 3)):
        key = F.forge_key(*shape)
        h0, h1 = F.honest(key, 300), F.honest(key, 301)
        kinds = [("Groth16", lambda c, t: shift_groth(key, c, t), R.PAIRING)]
        if key["n_commitments"]:
            kinds.append(("Pedersen", shift_pedersen, R.PEDERSEN))
        for what, shift, verdict in kinds:
            pair = [shift(h0, T), shift(h1, -T)]
            for i, c in enumerate(pair):
                out.append(_batch(f"{what} defect {'+-'[i]}t alone", key, [c], SEED_A, (verdict, 1)))
            out.append(_batch(f"{what} defects +t and -t", key, pair, SEED_A, (verdict, 2)))
            weighted = [shift(h0, r1 * T), shift(h1, -r0 * T)]
            out.append(_batch(f"{what} defects r_1 t and -r_0 t under their seed", key, weighted, SEED_A, (R.OK, 2), crafted_for_seed=True))
            out.append(_batch(f"{what} defects r_1 t and -r_0 t under another seed", key, weighted, SEED_B, (verdict, 2)))
    return out


def distinct_batches():
    """verify_forge.distinct_batch of 70: as it stands, without its malformed entries, without 31 (Groth16) as well, without 64
    (Pedersen) as well; then a second encoding inside the batch that fails with 1"""
    out = []
    for shape in ((3, 1), (3, 3)):
        key = F.forge_key(*shape)
        full = F.distinct_batch(key, 70, 700 + shape[1])
        keep = lambda drop: [c for i, c in enumerate(full) if i not in drop]
        out.append(_batch("70 distinct proofs", key, full, SEED_A, (R.MALFORMED, 0)))
        out.append(_batch("70 without 0, 63, 69", key, keep({0, 63, 69}), SEED_A, (R.PAIRING, 67)))
        out.append(_batch("70 without 0, 31, 63, 69", key, keep({0, 31, 63, 69}), SEED_A, (R.PEDERSEN, 66)))
        out.append(_batch("70 without 0, 31, 63, 64, 69", key, keep({0, 31, 63, 64, 69}), SEED_A, (R.OK, 65)))
        failing = keep({0, 63, 69})
        failing[40] = F.but(failing[40], words=[("raw", F.RAW["Krs.y"], F.p)])
        out.append(_batch("a second encoding at 40 of a failing batch", key, failing, SEED_A, (R.MALFORMED, 40)))
    return out


def all_batches():
    return accepted_batches() + single_batches() + cancelling_batches() + distinct_batches()
