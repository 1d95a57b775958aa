"""CPU suite: the library exports every symbol include/mi355x_groth16_verify.h declares (groth16.Verify on the device), the binding's
list matches the header, the binding's structures have the header's sizes, the header is product surface, and the two debug entry points
of the pairing are declared where the lab bench lives."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify.h")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_verify_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    for n in ("mi_vk_load", "mi_vk_free", "mi_pedersen_vk_make", "mi_groth16_verify", "mi_groth16_verify_batch"):
        assert n in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify.h but not exported"
    assert sorted(B.VERIFY_EXPORTS) == names
    assert not set(B.VERIFY_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS))


def test_verify_header_is_product_surface():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16.h", "mi355x_groth16_setup.h"]
    assert "hash" in src and "NOT PINNED" in src          # the caller hashes; the verifier is defined by its equations
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    B = load_binding()
    for n in ("mi_debug_pairing_dev", "mi_debug_fp12_op_dev"):
        assert n in dbg and n in B.EXPORTS and hasattr(B.load(), n)
    for h in ("mi355x_groth16.h", "mi355x_groth16_setup.h"):
        assert "mi_vk_load" not in open(os.path.join(ROOT, "include", h)).read()


def test_verify_binding_structures_match_the_header_layout():
    B = load_binding()
    assert C.sizeof(B.PedersenVk) == 2 * 128
    assert C.sizeof(B.VkDesc) == 64 + 3 * 128 + 8 + 8 + 4 + 4 + 8
    assert C.sizeof(B.VerifyInput) == (64 + 128 + 64) + 5 * 8
    src = open(HEADER).read()
    for name, val in (("MI_VERIFY_OK", B.VERIFY_OK), ("MI_VERIFY_PAIRING", B.VERIFY_PAIRING), ("MI_VERIFY_PEDERSEN", B.VERIFY_PEDERSEN),
                      ("MI_VERIFY_MALFORMED", B.VERIFY_MALFORMED)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == val
    dbg = open(os.path.join(ROOT, "include", "mi355x_groth16_debug.h")).read()
    assert int(re.search(r"#define MI_PAIRING_FINAL_EXP (\d+)u", dbg).group(1)) == B.PAIRING_FINAL_EXP


def test_verify_refuses_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context"""
    lib = load_binding().load()
    v = C.c_uint8()
    assert lib.mi_groth16_verify(None, None, None, C.byref(v)) == -1
    assert lib.mi_groth16_verify_batch(None, None, None, C.c_size_t(0), None) == -1
    assert lib.mi_vk_load(None, None, None) == -1 and lib.mi_pedersen_vk_make(None, None, C.c_uint32(0), None) == -1
