"""CPU suite: the library exports every symbol include/mi355x_groth16_verify_combined.h declares (one verdict for a batch of proofs), the
binding's list matches the header and is disjoint from the other lists, the header is product surface and states the semantics the tests
pin, the two debug entry points are declared where the lab bench lives, and null arguments are refused without a device."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify_combined.h")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_verify_combined_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert names == ["mi_groth16_verify_bytes_combined", "mi_groth16_verify_combined"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify_combined.h but not exported"
    assert sorted(B.VERIFY_COMBINED_EXPORTS) == names
    assert not set(B.VERIFY_COMBINED_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) |
                                                  set(B.VERIFY_BYTES_EXPORTS))


def test_verify_combined_header_is_product_surface_and_states_its_semantics():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_verify.h", "mi355x_groth16_verify_bytes.h"]
    for phrase in ('SHA-256("mi355x-g16-combine" | seed (32 bytes) | le64(n) | le64(i))', "first 16 bytes", "getrandom", "CANNOT PREDICT", "2^-128",
                   "lowest such index", "first_malformed = n", "do not say WHICH proof", "is always accepted"):
        assert phrase in src, phrase
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    B = load_binding()
    for n in ("mi_debug_fp12_product_dev", "mi_debug_g1_scale128_dev"):
        assert n in dbg and n in B.EXPORTS and hasattr(B.load(), n)
    for h in ("mi355x_groth16.h", "mi355x_groth16_setup.h", "mi355x_groth16_verify.h", "mi355x_groth16_verify_bytes.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert "_combined" not in text
    old = open(os.path.join(ROOT, "include", "mi355x_groth16_verify.h")).read()
    assert "mi355x_groth16_verify_combined.h" in old and "no random" not in old      # the old header points here


def test_verify_combined_refuses_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context"""
    lib = load_binding().load()
    v, first = C.c_uint8(255), C.c_uint64(77)
    assert lib.mi_groth16_verify_combined(None, None, None, C.c_size_t(0), None, C.byref(v), C.byref(first)) == -1
    assert lib.mi_groth16_verify_bytes_combined(None, None, None, C.c_size_t(0), None, C.byref(v), C.byref(first)) == -1
    assert (v.value, first.value) == (255, 77)
    assert lib.mi_debug_fp12_product_dev(None, None, C.c_size_t(1), None) == -1
    assert lib.mi_debug_g1_scale128_dev(None, None, None, C.c_size_t(1), None) == -1
