"""The locating batch verifier (include/mi355x_groth16_verify_locate.h) in the exponent, for tests/test_verify_locate_cpu.py and
tests/test_gpu_verify_locate.py.  Built on tests/verify_forge.py and tests/verify_combine_ref.py; nothing here calls the code under test.

A node of the tree (fan-in 8, node (l, j) = the proofs [j 8^l, min(n, (j + 1) 8^l))) passes when the defects of its well-formed proofs,
weighted by the coefficients of the WHOLE batch (coefficients(seed, n), original indices), sum to zero in both equations.  model() runs the
header's descent over those answers: which proofs end under suspicion, and the rounds, node tests and per-proof judgements it takes.  A
suspect's verdict is verify_forge.verdict_in_exponent; every other well-formed proof is 0; a malformed one is 3."""
import pairing_ref as R
import verify_forge as F
import verify_combine_ref as CR

r = F.r
FAN_IN = 8
DEFAULT_CAP = 64       # MI_LOCATE_ROUND_NODES


def level_counts(n):
    """nodes per level 0 .. L; L >= 1 (n = 1: one level of one node)"""
    cnt = [n]
    while True:
        cnt.append(-(-cnt[-1] // FAN_IN))
        if cnt[-1] <= 1:
            return cnt


def node_range(n, l, j):
    return range(j * FAN_IN ** l, min(n, (j + 1) * FAN_IN ** l))


def malformed(case):
    return bool(case["malformed"] or case["words"])


def expected_each(key, cases):
    return [F.verdict_in_exponent(key, c) for c in cases]


def node_fails(key, cases, rs, l, j):
    mine = [i for i in node_range(len(cases), l, j) if not malformed(cases[i])]
    if sum(rs[i] * CR.groth_defect(key, cases[i]) for i in mine) % r:
        return True
    return bool(sum(rs[i] * CR.pedersen_defect(key, cases[i]) for i in mine) % r)


def descend(n, well_formed, fails, cap=None):
    """fails(l, j) -> bool.  Returns (suspects, {"rounds", "nodes_tested"})"""
    cap = cap or DEFAULT_CAP
    cnt = level_counts(n)
    L = len(cnt) - 1
    if not any(well_formed):
        return [], {"rounds": 0, "nodes_tested": 0}
    st = {"rounds": 1, "nodes_tested": 1}
    if not fails(L, 0):
        return [], st
    failing, l = [0], L
    while l > 1:
        kids = lambda j, lo: range(j * FAN_IN ** (l - lo), min(cnt[lo], (j + 1) * FAN_IN ** (l - lo)))
        m = {lo: sum(len(kids(j, lo)) for j in failing) for lo in range(1, l)}
        lo = next((x for x in range(1, l) if m[x] <= cap), l - 1)
        u = sum(1 for j in failing for i in node_range(n, l, j) if well_formed[i])
        if u <= 2 * m[lo]:
            break
        st["rounds"] += 1
        st["nodes_tested"] += m[lo]
        nxt = []
        for j in failing:
            bad = [c for c in kids(j, lo) if fails(lo, c)]
            nxt += bad or list(kids(j, lo))          # every child passes: all of them stay under suspicion
        failing, l = nxt, lo
    return [i for j in failing for i in node_range(n, l, j) if well_formed[i]], st


def model(key, cases, seed, cap=None):
    """(verdicts, stats) the header promises for this batch under this seed"""
    n = len(cases)
    rs = CR.coefficients(seed, n)
    wf = [not malformed(c) for c in cases]
    suspects, st = descend(n, wf, lambda l, j: node_fails(key, cases, rs, l, j), cap)
    verdicts = [R.OK if ok else R.MALFORMED for ok in wf]
    for i in suspects:
        verdicts[i] = F.verdict_in_exponent(key, cases[i])
    st.update(judged_alone=len(suspects), malformed=wf.count(False), rejected=sum(v in (R.PAIRING, R.PEDERSEN) for v in verdicts))
    return verdicts, st
