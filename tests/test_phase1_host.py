"""CPU suite: the per-lane text of the phase-1 kernels and the contribution records (include/mi355x_groth16_phase1.h) on the host.
tests/cpp/phase1_host.cpp, its own main, built with -fsanitize=address,undefined by `make sanitize-phase1`, runs the recoding into
signed fixed-window digits, the per-lane table and the ladder of csrc/scale_powers.cuh -- the text phase1.hip's kernels run -- for
W = 2..5, G1 and G2, against xyzz_mul_256, and the chain of records of csrc/phase1_ops.cuh through mi_phase1_records_verify
(csrc/phase1_records.hip).  The program judges for itself and says what it ran; this file checks that it ran all of it.  No library is
preloaded anywhere."""
import os
import re
import subprocess
import pytest
from gpu_common import ROOT

N_SCALARS = 5 + 2 * 254 + 1 + 200   # 0, 1, 2, r - 1, r - 2; 2^j and 2^j - 1 for j <= 253; 2^254 - 1; 200 random


@pytest.fixture(scope="module")
def host_output():
    pkg = os.path.join(ROOT, "gnark-whir_amd")
    subprocess.check_call(["make", "-C", pkg, "-s", "sanitize-phase1"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(pkg, "build", "phase1_host_asan")], capture_output=True, text=True, env=env, timeout=900)
    assert res.returncode == 0 and not res.stderr.strip(), f"rc {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    assert "FAIL" not in res.stdout
    return res.stdout.splitlines()


def test_recoding_gives_the_scalar_back_for_every_width(host_output):
    for w in (2, 3, 4, 5):
        digits = -(-255 // w)
        assert f"recode W={w} digits={digits} scalars={N_SCALARS} bad=0" in host_output


def test_ladder_lane_equals_double_and_add_for_g1_and_g2(host_output):
    for group in ("G1", "G2"):
        ref = [l for l in host_output if l.startswith(f"reference {group} ")]
        assert len(ref) == 1
        at_inf = int(re.search(r"at_infinity=(\d+)", ref[0]).group(1))
        assert f"points={N_SCALARS}" in ref[0] and N_SCALARS // 5 <= at_inf < N_SCALARS // 2, "the point at infinity and the scalar 0 are among the cases, and not much else"
        for w in (2, 3, 4, 5):
            assert f"ladder {group} W={w} scalars={N_SCALARS} bad=0" in host_output


def test_record_chain_verifies_and_every_tamper_is_caught_where_it_is(host_output):
    # honest; 10 fields x 3 records; first_index, start_hash; two swaps; 4 x 3 of off-curve / infinity / infinity / response + r; continued; nulls
    assert f"chain cases={1 + 30 + 2 + 2 + 12 + 1 + 1}" in host_output
    assert host_output[-1] == "failures=0"
