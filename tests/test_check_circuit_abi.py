"""zg_prover_check_circuit / _dev through the layers that name them: the header, the built library, the Python binding's
symbol list and the generated Rust block.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("zg_prover_check_circuit", "zg_prover_check_circuit_dev")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_entries_and_the_fourth_kind():
    header = read("include", "zg_halo2.h")
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        args = decl.group(1)
        assert "const zg_fr *challenges" in args and "zg_failure *failures" in args and "uint32_t *totals" in args
    assert re.search(r"ZG_FAIL_SHUFFLE\s*=\s*3\b", header)


def test_library_exports_the_entries(zg):
    lib = zg.load()
    for name in ENTRIES:
        assert name in zg.ABI_SYMBOLS and hasattr(lib, name), name
    assert zg.FAIL_SHUFFLE == 3


def test_generated_rust_block_contains_the_entries():
    rust = read("shim", "halo2_proofs-zg", "src", "zg_sys.rs")
    for name in ENTRIES:
        assert re.search(r"pub fn %s\(" % name, rust), name
