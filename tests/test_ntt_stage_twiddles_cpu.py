"""CPU suite: NttPass::tw_stage (stage twiddles by global index, gnark-whir_amd/csrc/ntt_tile.cuh) on the host.  tests/emu/ntt_stage_tw.cpp
is a stand-alone program: it runs ntt_build_transform's records through ntt_tile_load / ntt_tile_stage / ntt_tile_store with the
stage-twiddle tables bound and compares, element by element, with the same records under the null pointer (tile-local twiddles and the
product at the pass's edge) -- 2^8 .. 2^13 under the plans (5, 4, 3) and (6, 5, 4) (one, two and three strided passes), all eight modes
(inverse, coset, DIF / DIT), n_valid < N -- and at 2^8 with the transform's definition (N^2 products).  Its last cases feed every input at
2p - 1 (DIF) and 4p - 1 (DIT) and check what every pass stores against the ranges the header documents: [0, 2p) and [0, 4p).  The build
traps on any violated bound of the lazy arithmetic (MI_CHECK_NOWRAP) and runs under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ntt_stage_tw") / "ntt_stage_tw")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMI_CHECK_NOWRAP", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "ntt_stage_tw.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


def test_stage_twiddles_match_the_edge_product_path_and_the_definition(driver_output):
    rc, out, err = driver_output
    assert rc == 0 and out.strip().endswith("ok") and "FAIL" not in out, (rc, out[-2000:], err[-2000:])


def test_every_required_case_ran(driver_output):
    """the driver's own list of cases: every size, both plans, all eight modes; one, two and three strided passes; both lazy edge cases"""
    _, out, _ = driver_output
    lines = [l for l in out.splitlines() if l.startswith("case ")]
    for log_n in range(8, 14):
        for plan in ("(5,4,3)", "(6,5,4)"):
            for flags in range(8):
                assert any(l.startswith(f"case log_n={log_n} plan={plan} flags={flags} ") for l in lines), (log_n, plan, flags)
    assert {int(l.rsplit("strided=", 1)[1]) for l in lines if "strided=" in l} >= {1, 2, 3}
    for dit in (0, 1):
        assert sum(l.startswith(f"case lazy dit={dit} ") for l in lines) >= 2
