"""CPU suite: the library exports every symbol include/mi355x_groth16_r1cs.h declares (the device-resident R1CS and the proofs from W
alone), the binding's list matches the header, the binding's structures have the header's sizes -- and the host reference the GPU tests
compare against (tests/r1cs_cases.py) is right: it reproduces pyref's solver on the toy circuits and Python integers on the skewed ones."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import pyref as P
import dlog_keys as D
import setup_cases as S
import r1cs_cases as RC
from helpers import fr_arr, fr_vals
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_r1cs.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_r1cs_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    for n in ("mi_r1cs_load", "mi_r1cs_eval_dev", "mi_r1cs_check_dev", "mi_groth16_prove_w", "mi_prover_submit_w_bsb22"):
        assert n in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_r1cs.h but not exported"
    assert sorted(B.R1CS_EXPORTS) == names
    assert not set(B.R1CS_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS))


def test_r1cs_header_is_product_surface():
    """no generator, probe or knob in it; it builds on the setup header alone, and the two older headers did not grow for it"""
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_setup.h"]
    for h in ("mi355x_groth16.h", "mi355x_groth16_setup.h"):
        assert "r1cs_load" not in open(os.path.join(ROOT, "include", h)).read()


def test_r1cs_binding_structures_match_the_header_layout():
    B = load_binding()
    assert C.sizeof(B.R1csStats) == 4 + 4 + 3 * 8
    src = open(HEADER).read()
    for name, val in (("MI_R1CS_A", B.R1CS_A), ("MI_R1CS_B", B.R1CS_B), ("MI_R1CS_C", B.R1CS_C), ("MI_PROVE_W_EVAL_C", B.PROVE_W_EVAL_C)):
        assert int(re.search(rf"#define {name} (\d+)u", src).group(1)) == val
    assert C.sizeof(B.R1csDesc) == 8 + 8 + 8 + 3 * 24 + 16 + 8 + 3 * 8      # the descriptor is the setup header's


# ---------------------------------------------------------------------------------------------------- the host reference
@pytest.mark.parametrize("small_frac", [0.0, 0.9])
@pytest.mark.parametrize("nc", [100, 1000, 4096])
def test_reference_reproduces_the_toy_solver(nc, small_frac):
    cs = P.ToyR1CS(nc, 5, nc + int(small_frac * 10), small_frac)
    w, a, b, c = cs.solve()
    r1cs = S.toy_r1cs(cs)
    W = fr_arr(w)
    got = RC.eval_all(r1cs, W)
    for have, want, name in zip(got, (a, b, c), "abc"):
        assert np.array_equal(have, fr_arr(want)), name
    assert RC.check_rows(*got) == (0, RC.U64_MAX)
    # one private wire that occurs in a constraint, changed: the rows the definition says
    j = max(next(iter(row[0])) for row in cs.rows)
    w2 = list(w); w2[j] = (w2[j] + 1) % P.R_MOD
    ev = lambda d: sum(k * w2[i] for i, k in d.items()) % P.R_MOD
    bad = [i for i, row in enumerate(cs.rows) if (ev(row[0]) * ev(row[1]) - ev(row[2])) % P.R_MOD]
    assert bad and RC.check_rows(*RC.eval_all(r1cs, fr_arr(w2))) == (len(bad), bad[0])


def test_reference_on_skewed_rows_against_python_integers():
    n = (1 << 13) - 37
    r1cs = RC.skewed_r1cs(n, nb_wires=(1 << 13) + 11, nb_public=9, seed=5)
    W = RC.witness(r1cs["nb_wires"], 6)
    got = dict(zip("ABC", RC.eval_all(r1cs, W)))
    rng = np.random.default_rng(7)
    for name in "ABC":
        lens = r1cs["lens"][name]
        at = r1cs["long_at"][name]
        assert [int(lens[at[L]]) for L in RC.LONG_LENS] == list(RC.LONG_LENS) and max(RC.LONG_LENS) >= 10 ** 5
        rows = [at[L] for L in RC.LONG_LENS] + [int(np.nonzero(lens == 0)[0][0])] + [int(x) for x in rng.integers(0, n, 40)]
        for i in rows:
            assert D._int(got[name][i]) == RC.row_by_integers(r1cs, name, W, i), f"{name} row {i} of {int(lens[i])} entries"
        assert not got[name][lens == 0].any()
    # the planted values are what the generator says: every class of coefficient is in use, duplicates exist
    assert fr_vals(r1cs["coeffs"][:5]) == [0, 1, P.R_MOD - 1, 2, P.R_MOD - 1]
    assert set(range(5)) <= set(int(x) for x in r1cs["A"][2][:2000])
    rp, col, _ = r1cs["B"]
    assert any(len(set(col[int(rp[i]):int(rp[i + 1])])) < int(rp[i + 1] - rp[i]) for i in range(200))
    n_long, n_pieces = RC.split_counts(r1cs)
    assert n_long == 3 * sum(L > RC.SHORT for L in RC.LONG_LENS) and n_pieces == 3 * sum(-(-L // RC.CHUNK) for L in RC.LONG_LENS if L > RC.SHORT)
