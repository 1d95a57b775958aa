"""Inputs and references shared by tests/test_vkfile_cpu.py and tests/test_gpu_vkfile.py: the Python writers of a verifying key's stream
(VerifyingKey.WriteTo / WriteRawTo as include/mi355x_groth16_vkfile.h states them, every point through keyfile_cases.g1_enc / g2_enc) and
of a witness's bytes, the four toy keys (verify_cases.toy_case), their proofs made acceptable FOR the BSB22 hashes the bytes path
computes, and the edge values of the witness decoder.  Nothing here calls the code under test."""
import functools
import os
import random
import struct
import subprocess
import pyref as P
import verify_cases as V
import bytes_cases as BC
import keyfile_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
r = P.R_MOD
RAW, COMPRESSED = K.RAW, K.COMPRESSED
KEY_SHAPES = ((1, 0), (5, 1), (3, 2), (33, 0))      # (nb_public, n_commitments)
GOLDEN_VK = os.path.join(HERE, "golden", "vk_toy_c1.compressed.bin")
GOLDEN_WITNESS = os.path.join(HERE, "golden", "vk_toy_c1.witness.bin")
WITNESS_EDGES = (0, 1, r - 1, r, r + 1, (1 << 256) - 1)      # the last three are not below r


def build_emu(so):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMI_CHECK_NOWRAP", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "emu", "emu_witness.cpp")])
    return so


def write_vk_stream(vk, ped=(), lists=None, encoding=COMPRESSED):
    """vk: pyref points alpha1, beta1, beta2, gamma2, delta1, delta2 and the list k; ped: [(G, GSigmaNeg)]; lists: one list of 1-based
    indices per Pedersen key (default: empty lists)"""
    g1 = lambda q: K.g1_enc(q, encoding)
    g2 = lambda q: K.g2_enc(q, encoding)
    lists = [[] for _ in ped] if lists is None else lists
    out = [g1(vk["alpha1"]), g1(vk["beta1"]), g2(vk["beta2"]), g2(vk["gamma2"]), g1(vk["delta1"]), g2(vk["delta2"])]
    out += [struct.pack(">I", len(vk["k"]))] + [g1(q) for q in vk["k"]]
    out += [struct.pack(">I", len(lists))] + [struct.pack(">I", len(l)) + b"".join(struct.pack(">Q", j) for j in l) for l in lists]
    out += [struct.pack(">I", len(ped))] + [g2(g) + g2(gs) for g, gs in ped]
    return b"".join(out)


def vk_stream_len(n_k, n_ped, n_indices, encoding):
    g1 = 32 if encoding == COMPRESSED else 64
    return 3 * g1 + 3 * 2 * g1 + 4 + n_k * g1 + 4 + 4 * n_ped + 8 * n_indices + 4 + n_ped * 4 * g1


def write_witness(values, n_secret=0, seed=5):
    """witness.WriteTo: the public values, then n_secret seeded secret ones"""
    rnd = random.Random(seed)
    vals = [int(v) for v in values] + [rnd.randrange(r) for _ in range(n_secret)]
    return struct.pack(">III", len(values), n_secret, len(vals)) + b"".join(v.to_bytes(32, "big") for v in vals)


def mont(v):
    """the Montgomery residue of the integer v: v 2^256 mod r"""
    return (v << 256) % r


@functools.lru_cache(maxsize=None)
def toy_key(nb_public, n_commitments):
    """verify_cases.toy_case of this shape with what a key FILE holds beside it: beta1, delta1, and the committed lists.  With two
    commitments the second commits to the first's value (index nb_public: the entry behind the public wires)."""
    case = V.toy_case(n_commitments, nb_constraints=max(12, nb_public + 4), nb_public=nb_public)
    td = case["td"]
    vk = dict(case["vk"], beta1=P.g1_mul(P.G1_GEN, td.beta), delta1=P.g1_mul(P.G1_GEN, td.delta))
    lists = [[1, 2], [nb_public]][:n_commitments] if n_commitments == 2 else [[nb_public - 1] for _ in range(n_commitments)]
    return dict(case, vk=vk), lists


def hashed(case, lists):
    """the case as the bytes path judges it, made ACCEPTABLE for it: commitment values and fold challenge are the BSB22 hashes (the
    toy circuit's own values of the commitment wires are not), Krs takes up the difference -- (h_k - w_k) K_k / delta in the exponent --
    and pok is folded with the hashed challenge"""
    q = r
    nc = len(case["commitments"])
    cv, fold = BC.bsb22_hashes(case["commitments"], case["public_inputs"], lists)
    if not nc:
        return dict(case)
    ar, bs, krs = case["proof"]
    nbp = case["vk"]["nb_public"]
    priv = list(range(nbp, case["cs"].nb_wires))
    for k in range(nc):
        cw = priv[3 * k + 2]
        krs = P.g1_add(krs, P.g1_neg(P.g1_mul(P.G1_GEN, (cv[k] - case["commitment_values"][k]) * case["exps"]["K"][cw] % q)))
    pok = None
    for k, c in enumerate(case["commitments"]):
        pok = P.g1_add(pok, P.g1_mul(c, case["sigmas"][k] * pow(fold, k, q) % q))
    return dict(case, proof=(ar, bs, krs), commitment_values=cv, fold_challenge=fold, pok=pok)


def with_k1_at_infinity(case):
    """the case under the key whose K[1] is infinity (gnark emits that for a public wire no constraint uses), its proof still
    accepted: kSum loses x_1 K_1 / gamma, Krs takes up x_1 K_1 / delta"""
    ar, bs, krs = case["proof"]
    k = case["vk"]["k"]
    krs = P.g1_add(krs, P.g1_mul(P.G1_GEN, case["public_inputs"][0] * case["exps"]["K"][1] % r))
    return dict(case, vk=dict(case["vk"], k=[k[0], None] + k[2:]), proof=(ar, bs, krs))


def proof_bytes(case):
    ar, bs, krs = case["proof"]
    return P.proof_bytes({"ar": ar, "bs": bs, "krs": krs}, case["commitments"], case["pok"])


def batch_of_nine(case, lists):
    """[(name, proof bytes, public inputs, verdict by the reference or 3 for what has no decoding)]: honest proofs, Krs tampered, pok
    tampered (with commitments), a point that does not decode, one changed public input.  The reference (pairings in Python) runs once
    per distinct proof."""
    import pairing_ref as R
    h = hashed(case, lists)
    nc = len(case["commitments"])
    ref = lambda c: V.ref_verdict(c, **dict(zip(("commitment_values", "fold_challenge"), BC.bsb22_hashes(c["commitments"], c["public_inputs"], lists))) if nc else {})
    ar, bs, krs = h["proof"]
    good = proof_bytes(h)
    pub = list(h["public_inputs"])
    bad_krs = dict(h, proof=(ar, bs, P.g1_add(krs, P.G1_GEN)))
    no_y = next(e for name, e, _ in BC.g1_edge_encodings() if name == "X without y")
    items = [("honest", good, pub, ref(h)), ("Krs tampered", proof_bytes(bad_krs), pub, ref(bad_krs))]
    if nc:
        bad_pok = dict(h, pok=P.g1_add(h["pok"], P.G1_GEN))
        items.append(("pok tampered", proof_bytes(bad_pok), pub, ref(bad_pok)))
    else:
        items.append(("honest again", good, pub, items[0][3]))
    items.append(("Ar does not decode", no_y + good[32:], pub, R.MALFORMED))
    items.append(("Bs with flag 00", good[:32] + bytes([good[32] & 0x3F]) + good[33:], pub, R.MALFORMED))
    if pub:
        other = [(pub[0] + 1) % r] + pub[1:]
        items.append(("one changed public input", good, other, ref(dict(h, public_inputs=other))))
    else:
        items.append(("honest, no public input to change", good, pub, items[0][3]))
    items += [items[0], items[1], items[0]]
    assert len(items) == 9 and items[0][3] == R.OK and items[1][3] == R.PAIRING
    return items
