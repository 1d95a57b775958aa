"""CPU suite: the library exports every symbol include/mi355x_groth16_verify_ksum.h declares, the binding's list matches the header and is
disjoint from the other lists, the header is product surface and states the default budget, the debug entry point, the knob and the
counters are declared where the lab bench lives, and null arguments are refused without a device."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_verify_ksum.h")
NAMES = ["mi_vk_ksum_batch", "mi_vk_ksum_batch_dev", "mi_vk_ksum_get_info", "mi_vk_ksum_prepare"]


def _text(path):
    return open(path).read()


def _declared(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", _text(path), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_ksum_symbol():
    B = load_binding()
    lib = B.load()
    assert _declared() == NAMES == sorted(B.VERIFY_KSUM_EXPORTS)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_verify_ksum.h but not exported"
    others = (set(B.EXPORTS) | set(B.SETUP_EXPORTS) | set(B.R1CS_EXPORTS) | set(B.VERIFY_EXPORTS) | set(B.VERIFY_BYTES_EXPORTS) |
              set(B.VERIFY_COMBINED_EXPORTS) | set(B.VERIFY_LOCATE_EXPORTS) | set(B.VERIFY_WAVE_EXPORTS))
    assert not set(B.VERIFY_KSUM_EXPORTS) & others


def test_header_is_product_surface_and_states_the_budget():
    B = load_binding()
    src = _text(HEADER)
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["mi355x_groth16_verify.h"]
    assert re.search(r"#define MI_KSUM_DEFAULT_TABLE_BYTES \(\(uint64_t\)64 << 20\)", src) and B.KSUM_DEFAULT_TABLE_BYTES == 64 << 20
    for phrase in ("64 MiB", "THE VERDICTS DO\n * NOT CHANGE", "mi_msm_g1_dev", "never fails because of the table", "n above 2^24", "ksum: ",
                   "n == 0 gives MI_OK", "mi_vk_free frees it"):
        assert phrase in src, phrase
    states = dict(re.findall(r"#define (MI_KSUM_[A-Z_]+) (\d)\b", src))
    assert {k: int(v) for k, v in states.items()} == {"MI_KSUM_NOT_BUILT": B.KSUM_NOT_BUILT, "MI_KSUM_READY": B.KSUM_READY, "MI_KSUM_OVER_BUDGET": B.KSUM_OVER_BUDGET,
                                                      "MI_KSUM_NO_MEMORY": B.KSUM_NO_MEMORY, "MI_KSUM_NO_BASES": B.KSUM_NO_BASES}
    # the info record of the binding has the header's fields in the header's order
    body = re.search(r"typedef struct mi_vk_ksum_info \{(.*?)\} mi_vk_ksum_info;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == [n for n, _ in B.VkKsumInfo._fields_]
    assert C.sizeof(B.VkKsumInfo) == 40


def test_debug_entry_point_knob_and_counters_live_in_the_debug_header_only():
    B = load_binding()
    dbg_path = os.path.join(ROOT, "include", "mi355x_groth16_debug.h")
    assert "mi_debug_verify_pairs_dev" in _declared(dbg_path) and "mi_debug_verify_pairs_dev" in B.EXPORTS
    assert hasattr(B.load(), "mi_debug_verify_pairs_dev")
    dbg = _text(dbg_path)
    for word in ('"verify_ksum" 0 | 1', '"verify_ksum_min_batch" 1..2^24','"verify_ksum_batches"', '"verify_ksum_launches"'):
        assert word in dbg, word
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "mi355x_groth16_debug.h":
            assert "mi_debug_verify_pairs_dev" not in re.sub(r"/\*.*?\*/", "", _text(os.path.join(ROOT, "include", h)), flags=re.S), h


def test_the_other_bindings_declare_the_calls():
    """the C++ wrapper and the Go shim (source only) name the four calls"""
    hpp = _text(os.path.join(ROOT, "gnark-whir_amd", "host", "groth16_mi355x.hpp"))
    go = _text(os.path.join(ROOT, "gnark-whir_amd", "go", "mi355x", "verify.go"))
    for n in NAMES:
        assert n in hpp, f"{n} missing from groth16_mi355x.hpp"
        assert n in go, f"{n} missing from the Go shim"
    assert "mi355x_groth16_verify_ksum.h" in hpp and "mi355x_groth16_verify_ksum.h" in go


def test_ksum_calls_refuse_null_arguments_before_any_device_work():
    """no GPU is needed to be refused: MI_EINVAL without a context, nothing written"""
    B = load_binding()
    lib = B.load()
    info = B.VkKsumInfo(); info.window_bits = 9; info.state = 9
    out = (C.c_uint64 * 8)(*([7] * 8))
    sc = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert lib.mi_vk_ksum_prepare(None, None, C.c_uint64(0)) == -1
    assert lib.mi_vk_ksum_get_info(None, None, C.byref(info)) == -1 and info.window_bits == 9 and info.state == 9
    assert lib.mi_vk_ksum_batch_dev(None, None, None, None, C.c_size_t(0), None) == -1
    assert lib.mi_vk_ksum_batch_dev(None, None, sc, None, C.c_size_t(1), out) == -1
    assert lib.mi_vk_ksum_batch(None, None, sc, None, C.c_size_t(1), out) == -1
    assert lib.mi_vk_ksum_batch(None, None, sc, None, C.c_size_t((1 << 24) + 1), out) == -1
    assert lib.mi_debug_verify_pairs_dev(None, None, None, C.c_size_t(1), out, out) == -1
    assert list(out) == [7] * 8
