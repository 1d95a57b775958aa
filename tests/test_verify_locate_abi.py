"""CPU suite: the library exports every symbol include/mi355x_groth16_verify_locate.h declares (one verdict per proof at the combined
test's price), the binding's list matches the header and is disjoint from the other lists, the header is product surface and states the
semantics the tests pin, the debug entry points are declared where the lab bench lives, and null arguments are refused without a device."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify_locate.h")
DEBUG_NAMES = ("mi_debug_g1_sum_tree_dev", "mi_debug_locate_points_dev", "mi_debug_locate_colsums_dev", "mi_debug_set_locate_round_nodes")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_verify_locate_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert names == ["mi_groth16_verify_bytes_locate", "mi_groth16_verify_locate"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify_locate.h but not exported"
    assert sorted(B.VERIFY_LOCATE_EXPORTS) == names
    assert not set(B.VERIFY_LOCATE_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) |
                                                set(B.VERIFY_BYTES_EXPORTS) | set(B.VERIFY_COMBINED_EXPORTS))


def test_verify_locate_header_is_product_surface_and_states_its_semantics():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_verify_combined.h"]
    for phrase in ("do not end the batch", "with certainty", "2^-128", "CANNOT PREDICT", "8n/7", "getrandom", "FULL n", "ORIGINAL index",
                   'SHA-256("mi355x-g16-combine" | seed (32 bytes) | le64(n) | le64(i))', "never from a node test", "MI_LOCATE_ROUND_NODES"):
        assert phrase in src, phrase
    assert "mi_verify_locate_stats" in src and all(f in src for f in ("rounds", "nodes_tested", "judged_alone", "malformed", "rejected"))
    assert _declared(os.path.join(ROOT, "include", "mi355x_groth16_verify_combined.h")) == ["mi_groth16_verify_bytes_combined", "mi_groth16_verify_combined"]


def test_debug_entry_points_live_in_the_debug_header_only():
    B = load_binding()
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    for n in DEBUG_NAMES:
        assert n in dbg and n in B.EXPORTS and hasattr(B.load(), n)
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "mi355x_groth16_debug.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not [n for n in DEBUG_NAMES if n in text], h


def test_verify_locate_refuses_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context, nothing written"""
    B = load_binding()
    lib = B.load()
    v, st = (C.c_uint8 * 4)(9, 9, 9, 9), B.VerifyLocateStats(7, 7, 7, 7, 7)
    assert lib.mi_groth16_verify_locate(None, None, None, C.c_size_t(0), None, v, C.byref(st)) == -1
    assert lib.mi_groth16_verify_bytes_locate(None, None, None, C.c_size_t(0), None, v, C.byref(st)) == -1
    assert lib.mi_groth16_verify_locate(None, None, None, C.c_size_t(4), None, v, C.byref(st)) == -1
    assert list(v) == [9] * 4 and st.as_dict() == dict.fromkeys(("rounds", "nodes_tested", "judged_alone", "malformed", "rejected"), 7)
    assert lib.mi_debug_g1_sum_tree_dev(None, None, C.c_size_t(1), None) == -1
    assert lib.mi_debug_locate_points_dev(None, None, None, None, None, None, C.c_uint32(0), C.c_size_t(1), None) == -1
    assert lib.mi_debug_locate_colsums_dev(None, None, C.c_uint32(0), None, C.c_size_t(1), C.c_uint32(0), None, C.c_size_t(1), None) == -1
    assert lib.mi_debug_set_locate_round_nodes(None, C.c_uint32(0)) == -1
