"""CPU suite: the library exports every symbol include/mi355x_groth16_verify_bytes.h declares (groth16.Verify from a proof's bytes), the
binding's list matches the header and is disjoint from the other lists, the header is product surface and says what is not pinned, the
three debug entry points are declared where the lab bench lives, and null arguments are refused without a device."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify_bytes.h")


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_verify_bytes_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    for n in ("mi_vk_set_public_committed", "mi_groth16_verify_bytes", "mi_groth16_verify_bytes_batch", "mi_proof_read", "mi_hash_to_field"):
        assert n in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify_bytes.h but not exported"
    assert sorted(B.VERIFY_BYTES_EXPORTS) == names
    assert not set(B.VERIFY_BYTES_EXPORTS) & (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS))


def test_verify_bytes_header_is_product_surface():
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_verify.h"]
    assert "NOT PINNED" in src and "verify one gnark proof first" in src and "64 ZERO BYTES" in src
    dbg = _declared(os.path.join(ROOT, "include", "mi355x_groth16_debug.h"))
    B = load_binding()
    for n in ("mi_debug_decode_g1_dev", "mi_debug_decode_g2_dev", "mi_debug_hash_to_field_dev"):
        assert n in dbg and n in B.EXPORTS and hasattr(B.load(), n)
    for h in ("mi355x_groth16.h", "mi355x_groth16_setup.h", "mi355x_groth16_verify.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert "mi_groth16_verify_bytes" not in text and "mi_proof_read" not in text
    assert C.sizeof(B.VerifyBytesInput) == 24


def test_verify_bytes_refuses_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context"""
    lib = load_binding().load()
    v = C.c_uint8()
    assert lib.mi_groth16_verify_bytes(None, None, None, C.c_size_t(164), None, C.byref(v)) == -1
    assert lib.mi_groth16_verify_bytes_batch(None, None, None, C.c_size_t(0), None) == -1
    assert lib.mi_vk_set_public_committed(None, None, None, None) == -1
    assert lib.mi_proof_read(None, C.c_size_t(0), C.c_uint32(0), None, None, None) == -1
    assert lib.mi_hash_to_field(None, C.c_size_t(0), None, C.c_size_t(0), None) == -1
    assert lib.mi_debug_decode_g1_dev(None, None, C.c_size_t(1), None, None) == -1
    assert lib.mi_debug_decode_g2_dev(None, None, C.c_size_t(1), None, None) == -1
    assert lib.mi_debug_hash_to_field_dev(None, None, C.c_uint32(1), None, C.c_size_t(0), C.c_size_t(1), None) == -1
