"""The sigma chain of a phase-2 ceremony (include/mi355x_groth16_phase2_check.h) restated in Python: hashlib for the hash and the
challenge, oracle/pyref.py's own group law over the twist for the points.  Everything is built from known exponents: the point
[-sigma_k]2 of a commitment is e_k g2 for an exponent e_k this side knows.  Shared by tests/test_phase2_sigma_cpu.py and
tests/test_gpu_phase2_sigma.py; nothing here touches the library."""
import hashlib
import numpy as np
import pyref as P
from helpers import fr_arr, fr_vals, g2_arr, g2_pts

R = P.R_MOD
WORDS = 36   # a mi_phase2_sigma_proof as uint64 words: g_sigma_neg (16), commit (16), response (4)


def step_hash(prev, index, befores, afters, commits):
    msg = b"mi355x-phase2-sigma-record" + prev + index.to_bytes(8, "little") + len(befores).to_bytes(4, "little")
    for b, a, t in zip(befores, afters, commits):
        msg += P.g2_compress(b) + P.g2_compress(a) + P.g2_compress(t)
    return hashlib.sha256(msg).digest()


def challenge(h):
    return int.from_bytes(hashlib.sha256(b"mi355x-phase2-sigma-challenge" + h).digest()[:16], "little")


def chain(ident, first_index, e_start, steps):
    """steps: per step a list of (s_k, nonce_k), one pair per commitment; e_start: the exponents of the points the chain starts from.
    -> [([(after_k, commit_k, z_k)], hash)], the exponents after the last step"""
    out = []
    e, prev = list(e_start), ident
    for i, step in enumerate(steps):
        befores = [P.g2_mul(P.G2_GEN, x) for x in e]
        afters = [P.g2_mul(P.G2_GEN, x * s % R) for x, (s, _) in zip(e, step)]
        commits = [P.g2_mul(P.G2_GEN, x * n % R) for x, (_, n) in zip(e, step)]
        h = step_hash(prev, first_index + i, befores, afters, commits)
        c = challenge(h)
        out.append(([(a, t, (n + c * s) % R) for a, t, (s, n) in zip(afters, commits, step)], h))
        e, prev = [x * s % R for x, (s, _) in zip(e, step)], h
    return out, e


def accepts(prev, index, befores, parts, h):
    """the acceptance rule, restated: the hash matches and [z_k] before_k = T_k + [c] after_k for every k"""
    afters, commits = [p[0] for p in parts], [p[1] for p in parts]
    if step_hash(prev, index, befores, afters, commits) != h:
        return False
    c = challenge(h)
    return all(P.g2_mul(b, z) == P.g2_add(t, P.g2_mul(a, c)) for b, (a, t, z) in zip(befores, parts))


def proofs_array(steps):
    """the restated steps as the library's words: (m, nc, WORDS) uint64, and the list of the m chain values"""
    nc = len(steps[0][0]) if steps else 1
    out = np.zeros((len(steps), nc, WORDS), np.uint64)
    for i, (parts, _) in enumerate(steps):
        for k, (after, commit, z) in enumerate(parts):
            out[i, k, :16] = g2_arr([after])[0]
            out[i, k, 16:32] = g2_arr([commit])[0]
            out[i, k, 32:] = fr_arr([z])[0]
    return out, [h for _, h in steps]


def parts_of(step):
    """one step of the library's words, (nc, WORDS) uint64 -> [(after_k, commit_k, z_k)] in pyref's points and plain integers"""
    return [(g2_pts(row[:16])[0], g2_pts(row[16:32])[0], fr_vals(row[32:])[0]) for row in np.asarray(step).reshape(-1, WORDS)]


def first_bad(start, start_hash, first_index, proofs, hashes):
    """mi_phase2_sigma_records_verify restated over the library's words (points that are on the twist and not at infinity)"""
    befores, prev = list(start), start_hash
    for i, (step, h) in enumerate(zip(proofs, hashes)):
        parts = parts_of(step)
        if not accepts(prev, first_index + i, befores, parts, h):
            return i
        befores, prev = [p[0] for p in parts], h
    return len(hashes)
