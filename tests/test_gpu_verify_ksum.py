"""GPU suite: the verdict-per-proof verifiers staged through the key's window table (include/mi355x_groth16_verify_ksum.h; the stage is
mi_verify_stage_pairs of csrc/verify.hip, the knob "verify_ksum").  Knob 1 sums every row over the table and lays the pairs out on the
device; knob 0 is one MSM per proof and the group law on the host, the yardstick.  Neither may change a word: the pairs of a staged
batch are compared byte for byte, and the verdicts of mi_groth16_verify_batch, _wave and _bytes_batch under both knobs with each other
and with the verdict computed in the exponent (tests/verify_forge.py)."""
import numpy as np
import pytest
import pairing_ref as R
import verify_cases as V
import verify_forge as F
import bytes_cases as BC
import ksum_cases as K
from gpu_common import load_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """the table from one proof on (the knob "verify_ksum_min_batch" at 1; its default has a test of its own below): a proof alone takes
    the stage under test"""
    B = load_binding()
    c = B.Context(0)
    c.set_knob("verify_ksum_min_batch", 1)
    yield c
    c.close()


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


def _under(ctx, knob, f, *args):
    ctx.set_knob("verify_ksum", knob)
    try:
        return f(*args)
    finally:
        ctx.set_knob("verify_ksum", 1)


def _malformed(key, seed):
    """an accepted proof with Ar.x + p: a second encoding, verdict 3 under any key"""
    c = F.but(F.honest(key, seed), words=[("raw", F.RAW["Ar.x"], F.p)])
    return dict(c, name="Ar.x + p", want=R.MALFORMED)


# ---------------------------------------------------------------------------------------------------- the pairs, word for word
@pytest.mark.parametrize("nc", [0, 1, 2])
def test_pairs_of_a_staged_batch_are_those_of_the_older_stage_byte_for_byte(ctx, nc):
    """toy proofs (tests/verify_cases.py): the proof, the same under another Krs and under other public inputs, and one with Ar off the
    curve whose pairs are infinities -- against knob 0 and, for the well-formed ones, against the pairs pyref lays out"""
    B = load_binding()
    case = V.toy_case(nc)
    d, nbp, ped = V.vk_arrays(case["vk"])
    vkh = ctx.vk_load(d, nbp, ped)
    try:
        import pyref as P
        others = [case, dict(case, proof=(case["proof"][0], case["proof"][1], P.g1_mul(P.G1_GEN, 1009))),
                  dict(case, public_inputs=[x + 1 for x in case["public_inputs"]]), dict(case, proof=((1, 3), case["proof"][1], case["proof"][2]))]
        proofs = [V.proof_dict(c) for c in others]
        assert vkh.ksum_info()["state"] == B.KSUM_NOT_BUILT
        p1, q1 = vkh.verify_pairs(proofs)
        assert vkh.ksum_info()["state"] == B.KSUM_READY and vkh.ksum_info()["window_bits"] == 8, "the first per-proof call builds the table"
        p0, q0 = _under(ctx, 0, vkh.verify_pairs, proofs)
        assert np.array_equal(p1, p0) and np.array_equal(q1, q0)
        for i, c in enumerate(others[:3]):
            want_p, want_q, _ = V.emu_pairs(c)
            assert np.array_equal(p1[i], want_p) and np.array_equal(q1[i], want_q), (nc, i)
        assert not p1[3].any() and not q1[3].any()
        one_p, one_q = vkh.verify_pairs(proofs[1:2])
        assert np.array_equal(one_p[0], p1[1]) and np.array_equal(one_q[0], q1[1])
        want = [V.ref_verdict(c) for c in others[:3]] + [R.MALFORMED]
        assert want[0] == R.OK and want[1] == want[2] == R.PAIRING
        for f in (vkh.verify_batch, vkh.verify_wave):
            assert list(f(proofs)) == want == list(_under(ctx, 0, f, proofs))
    finally:
        vkh.free()


# ---------------------------------------------------------------------------------------------------- forged, edge and non-reduced inputs
def _mine(key_id):
    mine = [c for c in F.cases() if c["key"]["id"] == key_id]
    assert mine
    return mine[0]["key"], mine


def _batch_of_65(key, mine):
    """the key's cases in turn, with malformed proofs first, last and adjacent"""
    batch = [mine[i % len(mine)] for i in range(65)]
    for i in (0, 30, 31, 64):
        batch[i] = _malformed(key, 500 + i)
    return batch


@pytest.mark.parametrize("body", ["batch", "wave"])
@pytest.mark.parametrize("key_id", F.CASE_KEY_IDS)
def test_forged_cases_alone_and_in_mixed_batches_of_65(ctx, forged_vk, key_id, body):
    key, mine = _mine(key_id)
    vkh = forged_vk(key)
    f = vkh.verify_batch if body == "batch" else vkh.verify_wave
    want = [F.verdict_in_exponent(key, c) for c in mine]
    assert want == [c["want"] for c in mine]
    inputs = [F.verify_input(c) for c in mine]
    for knob in (1, 0):
        alone = [int(_under(ctx, knob, f, [x])[0]) for x in inputs]
        assert alone == want, (knob, [(c["name"], g, w) for c, g, w in zip(mine, alone, want) if g != w])
    batch = _batch_of_65(key, mine)
    want65 = [F.verdict_in_exponent(key, c) for c in batch]
    assert [want65[i] for i in (0, 30, 31, 64)] == [R.MALFORMED] * 4
    in65 = [F.verify_input(c) for c in batch]
    got1, got0 = list(f(in65)), list(_under(ctx, 0, f, in65))
    assert got1 == want65 == got0, [(c["name"], a, b, w) for c, a, b, w in zip(batch, got1, got0, want65) if not a == b == w]


@pytest.mark.parametrize("key_id", F.CASE_KEY_IDS)
def test_forged_cases_from_bytes_alone_and_in_mixed_batches_of_65(ctx, forged_vk, key_id):
    """the cases that have an encoding, their commitment values and challenge the hashes of their commitments (tests/bytes_cases.py); a
    proof that does not decode (Ar's flag bits 00) first, last and adjacent"""
    key, mine = _mine(key_id)
    vkh = forged_vk(key)
    seen = [BC.rehashed(c) for c in mine if not BC.has_no_encoding(c)]
    want = [F.verdict_in_exponent(key, c) for c in seen]
    items = [(BC.proof_bytes_of(c), F.verify_input(c).get("public_inputs") if c["pub"] else None) for c in seen]
    for knob in (1, 0):
        alone = [int(_under(ctx, knob, vkh.verify_bytes_batch, [x])[0]) for x in items]
        assert alone == want, (knob, [(c["name"], g, w) for c, g, w in zip(seen, alone, want) if g != w])
    items65, want65 = [items[i % len(items)] for i in range(65)], [want[i % len(items)] for i in range(65)]
    for i in (0, 30, 31, 64):
        b = items65[i][0]
        items65[i], want65[i] = (bytes([b[0] & 0x3F]) + b[1:], items65[i][1]), R.MALFORMED
    got1, got0 = list(vkh.verify_bytes_batch(items65)), list(_under(ctx, 0, vkh.verify_bytes_batch, items65))
    assert got1 == want65 == got0


# ---------------------------------------------------------------------------------------------------- counters, budget, workspace
def test_counters_rise_by_one_batch_and_by_the_same_launches_for_1_and_130_proofs(ctx, forged_vk):
    """the claim that no launch count of the stage depends on n; knob 0 moves neither counter"""
    key = F.forge_key(3, 1)
    vkh = forged_vk(key)
    batch = [F.verify_input(F.honest(key, 900 + i)) for i in range(5)] * 26
    assert len(batch) == 130
    per_call = {}
    for n in (1, 130):
        for f in (vkh.verify_batch, vkh.verify_wave):
            b0, l0 = ctx.counter("verify_ksum_batches"), ctx.counter("verify_ksum_launches")
            assert list(f(batch[:n])) == [R.OK] * n
            assert ctx.counter("verify_ksum_batches") == b0 + 1
            per_call[(n, f.__name__)] = ctx.counter("verify_ksum_launches") - l0
    assert len(set(per_call.values())) == 1 and min(per_call.values()) > 0, per_call
    b0, l0 = ctx.counter("verify_ksum_batches"), ctx.counter("verify_ksum_launches")
    assert list(_under(ctx, 0, vkh.verify_batch, batch[:3])) == [R.OK] * 3
    assert (ctx.counter("verify_ksum_batches"), ctx.counter("verify_ksum_launches")) == (b0, l0)


def test_by_default_batches_below_8_proofs_keep_the_older_stage():
    """a context of its own with no knob set: 7 proofs neither build nor use the table, 8 do (profiles/verify.txt has the pairs that
    chose the threshold); the verdicts are the same"""
    B = load_binding()
    c = B.Context(0)
    key = F.forge_key(3, 1)
    d, nbp, ped = V.vk_arrays(key["vk"])
    vkh = c.vk_load(d, nbp, ped)
    try:
        inputs = [F.verify_input(F.honest(key, 950 + i)) for i in range(8)]
        for f in (vkh.verify_batch, vkh.verify_wave):
            assert list(f(inputs[:7])) == [R.OK] * 7
        assert c.counter("verify_ksum_batches") == 0 and vkh.ksum_info()["state"] == B.KSUM_NOT_BUILT
        for f in (vkh.verify_batch, vkh.verify_wave):
            assert list(f(inputs)) == [R.OK] * 8
        assert c.counter("verify_ksum_batches") == 2 and vkh.ksum_info()["state"] == B.KSUM_READY
        assert list(vkh.verify_wave(inputs[:1])) == [R.OK] and c.counter("verify_ksum_batches") == 2
        with pytest.raises(B.MiError, match="verify_ksum_min_batch"):
            c.set_knob("verify_ksum_min_batch", 0)
    finally:
        vkh.free()
        c.close()


def test_a_key_whose_table_does_not_fit_stays_on_the_older_stage(ctx):
    B = load_binding()
    key = F.forge_key(3, 3)
    d, nbp, ped = V.vk_arrays(key["vk"])
    vkh = ctx.vk_load(d, nbp, ped)
    try:
        info = vkh.ksum_prepare(1000)
        assert (info["window_bits"], info["table_bytes"], info["state"], info["bases"]) == (0, 0, B.KSUM_OVER_BUDGET, 5)
        cases = F.distinct_batch(key, 70, 703)
        want = [F.verdict_in_exponent(key, c) for c in cases]
        inputs = [F.verify_input(c) for c in cases]
        b0 = ctx.counter("verify_ksum_batches")
        assert list(vkh.verify_batch(inputs)) == want == list(vkh.verify_wave(inputs))
        assert ctx.counter("verify_ksum_batches") == b0 and vkh.ksum_info()["state"] == B.KSUM_OVER_BUDGET
        assert vkh.ksum_prepare(K.budget_for(5, 4))["window_bits"] == 4
        assert list(vkh.verify_batch(inputs)) == want == list(vkh.verify_wave(inputs))
        assert ctx.counter("verify_ksum_batches") == b0 + 2
    finally:
        vkh.free()


def test_after_a_trim_and_a_small_batch_after_a_large_one(ctx, forged_vk):
    key = F.forge_key(3, 3)
    vkh = forged_vk(key)
    cases = F.distinct_batch(key, 70, 703)
    want = [F.verdict_in_exponent(key, c) for c in cases]
    inputs = [F.verify_input(c) for c in cases]
    assert list(vkh.verify_wave(inputs)) == want
    for lo, hi in ((62, 65), (0, 1), (69, 70)):
        assert list(vkh.verify_batch(inputs[lo:hi])) == want[lo:hi] == list(vkh.verify_wave(inputs[lo:hi]))
    before = ctx.mem_ledger()
    assert list(vkh.verify_batch(inputs)) == want and ctx.mem_ledger() == before, "nothing is allocated in steady state"
    ctx.trim()
    assert list(vkh.verify_batch(inputs[:3])) == want[:3]
    assert list(vkh.verify_wave(inputs)) == want
