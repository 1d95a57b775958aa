"""CPU suite: the library exports every symbol include/mi355x_groth16_verify_wave.h declares (the verifier with one wave per pairing),
the binding's list matches the header and is disjoint from the other lists, the header is product surface and says what the calls are
for, the debug entry points are declared where the lab bench lives, and null arguments are refused without a device."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify_wave.h")
DEBUG_NAMES = ("mi_debug_pairing_wave_dev", "mi_debug_fp12_op_wave_dev", "mi_debug_verify_wave_split")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_verify_wave_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert names == ["mi_groth16_verify_bytes_wave", "mi_groth16_verify_wave"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify_wave.h but not exported"
    assert sorted(B.VERIFY_WAVE_EXPORTS) == names
    assert not set(B.VERIFY_WAVE_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) |
                                             set(B.VERIFY_BYTES_EXPORTS) | set(B.VERIFY_COMBINED_EXPORTS) | set(B.VERIFY_LOCATE_EXPORTS))


def test_verify_wave_header_is_product_surface_and_says_what_the_calls_are_for():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_verify.h", "mi355x_groth16_verify_bytes.h"]
    for phrase in ("byte for byte", "mi_groth16_verify_batch", "mi_groth16_verify_combined", "mi_groth16_verify_locate", "large batches",
                   "verify wave: ", "n == 0 gives MI_OK", "may alternate"):
        assert phrase in src, phrase
    assert "MEASURED_RANGE_BELOW" not in src and re.search(r"n = \d+", src), "the header quotes the measured range"
    assert "CPU" not in src       # no comparison with a CPU verifier: none exists here


def test_debug_entry_points_live_in_the_debug_header_only():
    B = load_binding()
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    for n in DEBUG_NAMES:
        assert n in dbg and n in B.EXPORTS and hasattr(B.load(), n)
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "mi355x_groth16_debug.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not [n for n in DEBUG_NAMES if n in text], h


def test_verify_wave_refuses_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context, nothing written"""
    B = load_binding()
    lib = B.load()
    v = (C.c_uint8 * 4)(9, 9, 9, 9)
    ms = (C.c_float * 5)(7, 7, 7, 7, 7)
    assert lib.mi_groth16_verify_wave(None, None, None, C.c_size_t(0), v) == -1
    assert lib.mi_groth16_verify_bytes_wave(None, None, None, C.c_size_t(0), v) == -1
    assert lib.mi_groth16_verify_wave(None, None, None, C.c_size_t(4), v) == -1
    assert lib.mi_debug_verify_wave_split(None, None, None, C.c_size_t(4), v, ms) == -1
    assert list(v) == [9] * 4 and list(ms) == [7.0] * 5
    assert lib.mi_debug_pairing_wave_dev(None, None, None, C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.mi_debug_fp12_op_wave_dev(None, C.c_int(0), None, None, None, C.c_size_t(1)) == -1
