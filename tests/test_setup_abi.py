"""CPU suite: the library exports every symbol include/mi355x_groth16_setup.h declares (groth16.Setup on the device), the binding's
setup list matches the header, and the binding's structures have the sizes the header's have."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_setup.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_setup_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert "mi_groth16_setup" in names and "mi_groth16_setup_exponents" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_setup.h but not exported"
    assert sorted(B.SETUP_EXPORTS) == names
    assert not set(B.SETUP_EXPORTS) & set(B.EXPORTS)


def test_setup_header_is_product_surface():
    """no generator, probe or knob in it, and it builds on the product header alone"""
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert '#include "mi355x_groth16.h"' in src and "mi355x_groth16_debug.h" not in src


def test_binding_structures_match_the_header_layout():
    B = load_binding()
    assert C.sizeof(B.R1csMatrix) == 24
    assert C.sizeof(B.R1csDesc) == 8 + 8 + 8 + 3 * 24 + 16 + 8 + 3 * 8
    assert C.sizeof(B.Trapdoor) == 32 * (5 + B.MAX_COMMITMENTS)
    assert C.sizeof(B.VkOut) == 64 + 3 * 128 + 24
    assert C.sizeof(B.SetupExponents) == 8 * 8
    assert C.sizeof(B.SetupStats) == 9 * 4 + 4 + 3 * 8
    assert int(re.search(r"#define MI_PK_RAW_MAX_COMMITMENTS (\d+)", open(os.path.join(ROOT, "include", "mi355x_groth16.h")).read()).group(1)) == B.MAX_COMMITMENTS
