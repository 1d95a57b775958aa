"""CPU suite: the library exports every symbol include/mi355x_groth16_phase2.h declares (the keys from a powers-of-tau SRS), the binding's
list matches the header, the binding's structures have the sizes the header's have, and the header says what it leaves out."""
import ctypes as C
import os
import re
from gpu_common import load_binding, ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_groth16_phase2.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_phase2_symbol():
    B = load_binding()
    lib = B.load()
    names = _declared()
    assert "mi_phase2_init" in names and "mi_phase2_contribute" in names and "mi_phase2_seal" in names and "mi_phase2_to_streams" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mi355x_groth16_phase2.h but not exported"
    assert sorted(B.PHASE2_EXPORTS) == names
    assert not set(B.PHASE2_EXPORTS) & set(B.EXPORTS)


def test_phase2_header_is_product_surface():
    """no generator, probe or knob in it, no debug header under it, and the three things it does not do are named"""
    src = open(HEADER).read()
    assert not [n for n in _declared() if n.startswith(("mi_debug_", "mi_bench_", "mi_gen_"))]
    assert '#include "mi355x_groth16_setup.h"' in src and "mi355x_groth16_debug.h" not in src
    flat = " ".join(src.split())
    assert "NOT DONE HERE" in flat
    for phrase in ("pairing check that the SRS rows are consistent powers", "proofs of knowledge", "mpcsetup file formats", "NOT AVAILABLE"):
        assert phrase in flat, phrase


def test_binding_structures_match_the_header_layout():
    B = load_binding()
    assert C.sizeof(B.SrsDesc) == 4 * 8 + 128 + 4 * 8
    assert C.sizeof(B.Phase2Stats) == 9 * 4 + 4 + 4 * 8
    src = open(HEADER).read()
    for name in ("G1_A", "G1_B", "G2_B", "G1_K", "G1_Z", "VK_K", "BASIS"):
        assert int(re.search(rf"#define MI_PHASE2_{name} (\d+)u", src).group(1)) == getattr(B, "PHASE2_" + name)
