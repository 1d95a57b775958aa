"""A forger in the exponent for the verifier tests (tests/test_verify_edges_cpu.py, tests/test_gpu_verify.py).  Nothing here calls the code
under test.

Groth16's equation and the Pedersen check are linear in the exponent: with every discrete log of the key known, a proof that satisfies
them is two divisions mod r away, for ANY public inputs and ANY commitments -- no circuit -- and the verdict of any input is a few
integer operations:
    a b = alpha beta + ksum gamma + krs delta,   ksum = K[0] + sum_i x_i K[1+i] + sum_k h_k K[nb_public+k] + sum_k m_k      else 1
    pok = sum_k sigma_k c^k m_k                                                                                             else 2
(lower case = discrete logs to the generators; infinity has the exponent 0).  Verdict 3 comes from the case's STRUCTURE, never from
arithmetic: a point named off its curve or outside the r-torsion, or a word that is not below its modulus.

A key is forge_key's dict (its "vk" is what pairing_ref.groth16_verify and verify_cases.vk_arrays take).  A case is forge_proof's dict of
exponents; verify_input(case) makes what binding.VerifyingKey.verify takes and ref_args(case) what pairing_ref.groth16_verify takes,
both when they are asked for, and points come out of one cache (most cases share theirs)."""
import functools
import random
import numpy as np
import cref
import pyref as P
import pairing_ref as R
import verify_cases as V
from helpers import fr_arr, g1_arr, g2_arr

p, r = P.Q_MOD, P.R_MOD
B_POOL = (1, 2, 0x1234567, r - 1)   # the discrete logs Bs is drawn from: G2 multiples are the expensive ones


@functools.lru_cache(maxsize=None)
def g1(e):
    return P.g1_mul(P.G1_GEN, e % r) if e % r else None


@functools.lru_cache(maxsize=None)
def g2(e):
    return P.g2_mul(P.G2_GEN, e % r) if e % r else None


def inv(x):
    return pow(x % r, -1, r)


# ---------------------------------------------------------------------------------------------------- keys and proofs
KEY_SHAPES = ((1, 0), (2, 0), (3, 1), (3, 3), (2, 16))
CASE_KEYS = tuple((s, ()) for s in KEY_SHAPES) + (((2, 0), (1,)), ((3, 1), (0,)))    # (shape, zero_k) of every key of cases()


def key_id(nb_public, n_commitments, zero_k=()):
    return f"{nb_public}pub_{n_commitments}com" + "".join(f"_K{j}inf" for j in zero_k)


CASE_KEY_IDS = tuple(key_id(*s, z) for s, z in CASE_KEYS)


@functools.lru_cache(maxsize=None)
def forge_key(nb_public, n_commitments, seed=1, zero_k=()):
    """random exponents for alpha, beta, gamma, delta, K[j], sigma_k; K[j] = infinity for j in zero_k (gnark emits that for a public
    wire no constraint uses)"""
    rnd = random.Random(1000 * seed + 10 * nb_public + n_commitments)
    e = {n: rnd.randrange(1, r) for n in ("alpha", "beta", "gamma", "delta")}
    e["k"] = [0 if j in zero_k else rnd.randrange(1, r) for j in range(nb_public + n_commitments)]
    e["sigma"] = [rnd.randrange(1, r) for _ in range(n_commitments)]
    vk = {"alpha1": g1(e["alpha"]), "beta2": g2(e["beta"]), "gamma2": g2(e["gamma"]), "delta2": g2(e["delta"]),
          "k": [g1(x) for x in e["k"]], "nb_public": nb_public, "ped": R.pedersen_vk(e["sigma"])}
    return {"exps": e, "vk": vk, "nb_public": nb_public, "n_commitments": n_commitments,
            "id": key_id(nb_public, n_commitments, zero_k)}


def msm_e(key, public_inputs, commit_values):
    k = key["exps"]["k"]
    return sum(x * kj for x, kj in zip(list(public_inputs) + list(commit_values), k[1:])) % r


def ksum_e(key, public_inputs, commit_values, commit_exps):
    return (key["exps"]["k"][0] + msm_e(key, public_inputs, commit_values) + sum(commit_exps)) % r


def pok_of(key, commit_exps, fold):
    c = 1 if key["n_commitments"] <= 1 else fold    # the challenge is not read with one commitment
    return sum(s * pow(c, k, r) * m for k, (s, m) in enumerate(zip(key["exps"]["sigma"], commit_exps))) % r


def forge_proof(key, public_inputs, commit_exps, commit_values, fold, a, b, krs=None):
    """The exponents of a proof both equations accept: krs = (a b - alpha beta - ksum gamma) / delta, pok = sum sigma_k c^k m_k.  Any
    exponent may be forced to 0 (infinity); with a = None, krs is taken as given and a = (alpha beta + ksum gamma + krs delta) / b."""
    e = key["exps"]
    assert len(public_inputs) == key["nb_public"] - 1 and len(commit_exps) == len(commit_values) == key["n_commitments"]
    rest = e["alpha"] * e["beta"] + ksum_e(key, public_inputs, commit_values, commit_exps) * e["gamma"]
    if a is None:
        a = (rest + krs * e["delta"]) * inv(b) % r
    else:
        krs = (a * b - rest) * inv(e["delta"]) % r
    return {"key": key, "pub": [x % r for x in public_inputs], "cm": [m % r for m in commit_exps], "cv": [h % r for h in commit_values],
            "fold": fold, "a": a % r, "b": b % r, "krs": krs % r, "pok": pok_of(key, commit_exps, fold), "points": {}, "words": [],
            "malformed": None}


def verdict_in_exponent(key, case):
    """3, 1, 2 or 0 in the order of include/mi355x_groth16_verify.h"""
    e = key["exps"]
    if case["malformed"] or case["words"]:
        return R.MALFORMED
    assert not case["points"], "a named point without a reason why it is malformed"
    rhs = e["alpha"] * e["beta"] + ksum_e(key, case["pub"], case["cv"], case["cm"]) * e["gamma"] + case["krs"] * e["delta"]
    if (case["a"] * case["b"] - rhs) % r:
        return R.PAIRING
    if key["n_commitments"] and (case["pok"] - pok_of(key, case["cm"], case["fold"])) % r:
        return R.PEDERSEN
    return R.OK


def but(case, **over):
    """a copy of the case with some fields replaced (its own lists: the original stays as it is)"""
    c = dict(case, points=dict(case["points"]), words=list(case["words"]))
    for n in ("pub", "cm", "cv"):
        c[n] = list(c[n])
    c.update(over)
    return c


# ---------------------------------------------------------------------------------------------------- a case -> what the judges take
def case_points(case):
    """Ar, Bs, Krs, the commitments and pok as pyref points: from the exponents, unless the case names a point of its own"""
    pts = {"ar": g1(case["a"]), "bs": g2(case["b"]), "krs": g1(case["krs"]), "pok": g1(case["pok"]), "cm": [g1(m) for m in case["cm"]]}
    for name, pt in case["points"].items():
        if isinstance(name, tuple):
            pts["cm"][name[1]] = pt
        else:
            pts[name] = pt
    return pts


WORD_FIELDS = {"raw": p, "pok": p, "commitments": p, "public_inputs": r, "commitment_values": r, "fold_challenge": r}


def verify_input(case):
    """what binding.VerifyingKey.verify takes.  case["words"] = [(field, i, value)]: element i (4 words) of that array becomes value + its
    Montgomery words read as an integer (value = the modulus: a second encoding of the same element), or value itself with i < 0 given
    as (field, ~i, value) -- checked here to lie in [modulus, 2^256)."""
    pts = case_points(case)
    nc = case["key"]["n_commitments"]
    d = {"raw": np.concatenate([g1_arr([pts["ar"]])[0], g2_arr([pts["bs"]])[0], g1_arr([pts["krs"]])[0]])}
    if case["pub"]:
        d["public_inputs"] = fr_arr(case["pub"])
    if nc:
        d.update(commitments=g1_arr(pts["cm"]), pok=g1_arr([pts["pok"]])[0], commitment_values=fr_arr(case["cv"]))
        if case["fold"] is not None:
            d["fold_challenge"] = fr_arr([case["fold"]])[0]
    for field, i, value in case["words"]:
        rows = d[field].reshape(-1, 4)
        new = value if i < 0 else cref.limbs_to_int(rows[i]) + value
        assert WORD_FIELDS[field] <= new < 1 << 256, (case["name"], field, i)
        rows[~i if i < 0 else i] = cref.int_to_limbs(new)
    return d


def ref_args(case):
    """(vk, proof, public_inputs, commitments, commitment_values, pok, fold_challenge) of pairing_ref.groth16_verify"""
    assert not case["words"], "the reference works on integers: it has no second encoding"
    pts = case_points(case)
    fold = case["fold"] if case["key"]["n_commitments"] > 1 else 1
    return case["key"]["vk"], (pts["ar"], pts["bs"], pts["krs"]), case["pub"], pts["cm"], case["cv"], pts["pok"], fold


# ---------------------------------------------------------------------------------------------------- the case list
ONES = (1 << 256) - 1
RAW = {"Ar.x": 0, "Ar.y": 1, "Bs.x.a0": 2, "Bs.x.a1": 3, "Bs.y.a0": 4, "Bs.y.a1": 5, "Krs.x": 6, "Krs.y": 7}   # rows of "raw"


@functools.lru_cache(maxsize=None)
def g1_off_curve():
    return (1, 3)


def honest(key, seed, **force):
    """an accepted proof of random exponents; force: any argument of forge_proof"""
    rnd = random.Random(seed)
    nbp, nc = key["nb_public"], key["n_commitments"]
    args = dict(public_inputs=[rnd.randrange(1, r) for _ in range(nbp - 1)], commit_exps=[rnd.randrange(1, r) for _ in range(nc)],
                commit_values=[rnd.randrange(1, r) for _ in range(nc)], fold=rnd.randrange(2, r) if nc else None,
                a=rnd.randrange(1, r), b=B_POOL[seed % len(B_POOL)])
    args.update(force)
    return forge_proof(key, **args)


def _tweaked(case, which):
    """one exponent of an accepted proof changed by 1, and the verdict the equations then give"""
    if which == "krs":
        return but(case, krs=(case["krs"] + 1) % r), R.PAIRING
    if which == "a":
        return but(case, a=(case["a"] + 1) % r), R.PAIRING
    if which == "pub":
        return but(case, pub=[(case["pub"][0] + 1) % r] + case["pub"][1:]), R.PAIRING
    if which == "cv":
        return but(case, cv=case["cv"][:-1] + [(case["cv"][-1] + 1) % r]), R.PAIRING
    if which == "cm":      # kSum moves with the commitment: the first equation fails before the second is asked
        return but(case, cm=case["cm"][:-1] + [(case["cm"][-1] + 1) % r]), R.PAIRING
    if which == "pok":
        return but(case, pok=(case["pok"] + 1) % r), R.PEDERSEN
    if which == "fold":    # the powers of c reach the Pedersen equation alone
        return but(case, fold=(case["fold"] + 1) % r), R.PEDERSEN
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def cases():
    """[case]: forge_proof's dict with "name", "kind" (one of each kind also goes through the definitional pairing) and "want", the
    verdict this list states for it.  verdict_in_exponent must agree with "want": the list is written down, the rule computes."""
    out = []

    def add(name, kind, case, want):
        out.append(dict(case, name=f"{case['key']['id']}: {name}", kind=kind, want=want))

    def accepted(name, case, tweak):
        add(name, name, case, R.OK)
        t, want = _tweaked(case, tweak)
        add(f"{name}, {tweak} + 1", f"{tweak} + 1 on an accepted proof", t, want)

    k10, k20, k31, k33, k216 = (forge_key(*s) for s in KEY_SHAPES)
    k20_k1inf, k31_k0inf = forge_key(2, 0, zero_k=(1,)), forge_key(3, 1, zero_k=(0,))
    tweaks = {k10["id"]: "krs", k20["id"]: "pub", k31["id"]: "pok", k33["id"]: "fold", k216["id"]: "pok", k20_k1inf["id"]: "a",
              k31_k0inf["id"]: "cv"}
    for i, key in enumerate((k10, k20, k31, k33, k216, k20_k1inf, k31_k0inf)):
        accepted("honest", honest(key, 10 + i), tweaks[key["id"]])
    add("honest, fold_challenge NULL", "fold_challenge NULL with one commitment", honest(k31, 17, fold=None), R.OK)

    # ---- the scalar part of kSum
    for i, key in enumerate((k20, k31, k33)):
        nbp, nc = key["nb_public"], key["n_commitments"]
        accepted("every scalar 0", honest(key, 20 + i, public_inputs=[0] * (nbp - 1), commit_values=[0] * nc), ("krs", "cm", "pok")[i])
    for i, key in enumerate((k20, k31)):
        ke = key["exps"]["k"]
        for sign, what in ((-1, "MSM part = -K[0]"), (1, "MSM part = +K[0]")):
            h = honest(key, 30 + i)
            rest = msm_e(key, [0] + h["pub"][1:], h["cv"])
            x0 = (sign * ke[0] - rest) * inv(ke[1]) % r
            c = honest(key, 30 + i, public_inputs=[x0] + h["pub"][1:])
            assert msm_e(key, c["pub"], c["cv"]) == sign * ke[0] % r
            accepted(what, c, ("pub", "cv")[i])
    c = honest(k20_k1inf, 40)
    assert c["pub"][0] and k20_k1inf["vk"]["k"][1] is None
    accepted("K[1] = infinity with a non-zero input", c, "pub")     # the input multiplies infinity: + 1 changes nothing
    out[-1]["want"] = R.OK
    accepted("K[0] = infinity", honest(k31_k0inf, 41), "pub")
    accepted("K[0] = infinity, every scalar 0", honest(k31_k0inf, 42, public_inputs=[0, 0], commit_values=[0]), "krs")
    for i, key in enumerate((k10, k20, k31)):
        accepted("Krs = infinity", honest(key, 50 + i, a=None, krs=0), ("krs", "a", "pok")[i])

    # ---- the commitments against the running sum K[0] + MSM part, and each other
    for i, key in enumerate((k31, k33)):
        h = honest(key, 60 + i)
        run = (key["exps"]["k"][0] + msm_e(key, h["pub"], h["cv"])) % r
        accepted("C_0 = the running sum", honest(key, 60 + i, commit_exps=[run] + h["cm"][1:]), ("pok", "cm")[i])
        accepted("C_0 = -(the running sum)", honest(key, 60 + i, commit_exps=[-run % r] + h["cm"][1:]), ("krs", "pok")[i])
        accepted("C_0 = infinity", honest(key, 60 + i, commit_exps=[0] + h["cm"][1:]), ("pok", "fold")[i])
    h = honest(k33, 70)
    accepted("C_0 == C_1", honest(k33, 70, commit_exps=[h["cm"][0], h["cm"][0], h["cm"][2]]), "fold")
    run = (k33["exps"]["k"][0] + msm_e(k33, h["pub"], h["cv"]) + h["cm"][0]) % r
    accepted("C_1 = the running sum with C_0", honest(k33, 70, commit_exps=[h["cm"][0], run, h["cm"][2]]), "pok")
    accepted("C_1 = -(the running sum with C_0)", honest(k33, 70, commit_exps=[h["cm"][0], -run % r, h["cm"][2]]), "cm")
    s, c = k33["exps"]["sigma"], h["fold"]
    m2 = -(s[0] * h["cm"][0] + s[1] * c * h["cm"][1]) * inv(s[2] * c * c) % r
    c0 = honest(k33, 70, commit_exps=[h["cm"][0], h["cm"][1], m2])
    assert c0["pok"] == 0 and all(c0["cm"])
    accepted("pok = infinity, the weighted exponents sum to 0", c0, "pok")
    for i, key in enumerate((k33, k216)):
        for j, (c, what) in enumerate(((0, "0"), (1, "1"), (r - 1, "r - 1"))):
            accepted(f"fold_challenge = {what}", honest(key, 80 + 3 * i + j, fold=c), ("pok", "cm", "krs")[j])
    for i, key in enumerate((k33, k216)):     # every power c^2 .. c^15 with a small c: one dropped or repeated multiplication shows
        accepted("fold_challenge = 2", honest(key, 88 + i, fold=2), "fold")

    # ---- rejections by the equations
    for i, key in enumerate((k20, k33)):
        h = honest(key, 90 + i)
        add("Ar = infinity", "Ar = infinity", but(h, a=0), R.PAIRING)
        add("Bs = infinity", "Bs = infinity", but(h, b=0), R.PAIRING)
        add("-Ar", "-Ar", but(h, a=-h["a"] % r), R.PAIRING)
        add("Ar and Krs swapped", "Ar and Krs swapped", but(h, a=h["krs"], krs=h["a"]), R.PAIRING)
    h = honest(k31, 95)
    add("both equations fail", "both equations fail", but(h, krs=(h["krs"] + 1) % r, pok=(h["pok"] + 1) % r), R.PAIRING)

    # ---- malformed by a point, alone and together with a failing equation
    outside = V.twist_point_outside_subgroup()
    for i, key in enumerate((k20, k33)):
        h = honest(key, 100 + i)
        add("Ar off the curve", "Ar off the curve", but(h, points={"ar": g1_off_curve()}, malformed="off the curve"), R.MALFORMED)
        add("Krs off the curve", "Krs off the curve", but(h, points={"krs": g1_off_curve()}, malformed="off the curve"), R.MALFORMED)
        add("Bs outside the r-torsion", "Bs outside the r-torsion", but(h, points={"bs": outside}, malformed="outside the r-torsion"), R.MALFORMED)
        add("Bs off the twist", "Bs off the twist", but(h, points={"bs": ((1, 2), (3, 4))}, malformed="off the twist"), R.MALFORMED)
        add("Ar off the curve and Krs + 1", "malformed and a failing equation",
            but(h, krs=(h["krs"] + 1) % r, points={"ar": g1_off_curve()}, malformed="off the curve"), R.MALFORMED)
    h = honest(k33, 102)
    add("pok off the curve", "pok off the curve", but(h, points={"pok": g1_off_curve()}, malformed="off the curve"), R.MALFORMED)
    add("C_2 off the curve", "a commitment off the curve", but(h, points={("cm", 2): g1_off_curve()}, malformed="off the curve"), R.MALFORMED)
    add("Bs outside the r-torsion and pok + 1", "malformed and a failing Pedersen equation",
        but(h, pok=(h["pok"] + 1) % r, points={"bs": outside}, malformed="outside the r-torsion"), R.MALFORMED)

    # ---- second encodings: an accepted proof with ONE element's words not reduced
    h = honest(k33, 110)
    assert verdict_in_exponent(k33, h) == R.OK
    for what, word in (("Ar.x + p", ("raw", RAW["Ar.x"], p)), ("Ar.y + p", ("raw", RAW["Ar.y"], p)), ("Bs.x.a1 + p", ("raw", RAW["Bs.x.a1"], p)),
                       ("Bs.y.a0 + p", ("raw", RAW["Bs.y.a0"], p)), ("Krs.y + p", ("raw", RAW["Krs.y"], p)), ("pok.x + p", ("pok", 0, p)),
                       ("C_1.y + p", ("commitments", 3, p)), ("public_inputs[1] + r", ("public_inputs", 1, r)),
                       ("commitment_values[2] + r", ("commitment_values", 2, r)), ("fold_challenge + r", ("fold_challenge", 0, r)),
                       ("Ar.x = 2^256 - 1", ("raw", ~RAW["Ar.x"], ONES)), ("public_inputs[0] = 2^256 - 1", ("public_inputs", ~0, ONES)),
                       ("pok.y = p", ("pok", ~1, p)), ("fold_challenge = r", ("fold_challenge", ~0, r))):
        add(what, "not reduced", but(h, words=[word]), R.MALFORMED)
    add("Ar = (p, p)", "not reduced", but(h, words=[("raw", ~RAW["Ar.x"], p), ("raw", ~RAW["Ar.y"], p)]), R.MALFORMED)
    add("Bs = (p, p, p, p)", "not reduced", but(h, words=[("raw", ~RAW[n], p) for n in ("Bs.x.a0", "Bs.x.a1", "Bs.y.a0", "Bs.y.a1")]), R.MALFORMED)
    h = honest(k20, 111)
    add("public_inputs[0] + r", "not reduced", but(h, words=[("public_inputs", 0, r)]), R.MALFORMED)
    add("Krs.x + p", "not reduced", but(h, words=[("raw", RAW["Krs.x"], p)]), R.MALFORMED)
    h = honest(k31, 112)
    add("commitment_values[0] + r", "not reduced", but(h, words=[("commitment_values", 0, r)]), R.MALFORMED)
    add("C_0.x + p", "not reduced", but(h, words=[("commitments", 0, p)]), R.MALFORMED)
    return out


def keys_of(case_list):
    """the distinct keys of a case list, in order of appearance"""
    seen = {}
    for c in case_list:
        seen.setdefault(c["key"]["id"], c["key"])
    return list(seen.values())


# ---------------------------------------------------------------------------------------------------- a batch of distinct proofs
def distinct_batch(key, n, seed):
    """n cases for one key, every one with its own public inputs, commitment values and a; rejections of all three kinds at 0, 63, 64
    and n - 1 (Bs outside the r-torsion, Ar not reduced, a Pedersen failure, Bs outside the r-torsion again), and at 31 the proof of 30
    with other public inputs (rejected: the proof is bound to them)"""
    assert n > 64 and key["n_commitments"]
    out = [dict(honest(key, seed + i), name=f"batch entry {i}") for i in range(n)]
    outside = V.twist_point_outside_subgroup()
    out[0] = but(out[0], points={"bs": outside}, malformed="outside the r-torsion")
    out[63] = but(out[63], words=[("raw", RAW["Ar.x"], p)])
    out[64] = but(out[64], pok=(out[64]["pok"] + 1) % r)
    out[n - 1] = but(out[n - 1], points={"bs": outside}, malformed="outside the r-torsion")
    out[31] = but(out[30], pub=out[31]["pub"], name="batch entry 31: the proof of 30, other public inputs")
    return out
