"""Host side of the keygen entries (no GPU): the two coset generators zg_fr_cube_root hands out, against Python integers,
and the header's account of every entry that came with them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ["zg_fr_cube_root", "zg_ctx_set_coset_generator", "zg_ctx_coset_generator", "zg_prover_coset_generator",
               "zg_permutation_sigma", "zg_prover_export_key"]
KEY_FAMILIES = ["ZG_KEY_FIXED_POLY", "ZG_KEY_SIGMA_POLY", "ZG_KEY_FIXED_COSET", "ZG_KEY_SIGMA_COSET", "ZG_KEY_L0", "ZG_KEY_L_LAST",
                "ZG_KEY_L_ACTIVE_ROW"]


def test_both_cube_roots_match_python_integers(zg):
    R = zg.FR_MODULUS
    z0, z1 = zg.fr_to_int(zg.fr_cube_root(0)), zg.fr_to_int(zg.fr_cube_root(1))
    assert z0 == pow(7, (R - 1) // 3, R)
    assert z0 & 0xFFFFFFFF == 0xB99C90DD
    assert z1 == z0 * z0 % R == 0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23
    for z in (z0, z1):
        assert z != 1 and pow(z, 3, R) == 1
    assert z0 != z1 and z1 * z1 % R == z0
    assert zg.fr_to_int(zg.fr_cube_root()) == z0  # (the default)
    import pytest

    with pytest.raises(zg.ZgError) as e:
        zg.fr_cube_root(2)
    assert e.value.status == -1


def test_header_documents_every_new_entry():
    text = open(os.path.join(ROOT, "include", "zg_halo2.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    assert "evaluation domain" in comments
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
    # every entry stands under a comment of its own (the getter under its setter's; export_key under its families, which stand
    # under the comment)
    for name in NEW_ENTRIES:
        before = text[:re.search(r"\bint %s\s*\(" % name, text).start()].rstrip()
        if name == "zg_ctx_coset_generator":
            assert re.search(r"int zg_ctx_set_coset_generator\([^;]*\);$", before), name
        elif name == "zg_prover_export_key":
            assert re.search(r"\*/\s*enum \{[^}]*ZG_KEY_L_ACTIVE_ROW[^}]*\};$", before), name
        else:
            assert before.endswith("*/"), name
    for fam in KEY_FAMILIES:
        assert re.search(r"\b%s\s*=\s*\d" % fam, code), fam
        assert fam in comments, fam
    # which value is the default and why; what a shim passes
    section = re.sub(r"\s*\n \*\s*", " ", text[text.index("evaluation domain"):text.index("circuit description")])  # (lines rejoined)
    for phrase in ("DEFAULT", "7^((r-1)/3)", "golden vectors", "not been verified", "WithSmallOrderMulGroup<3>>::ZETA", "ZG_ERR_INVALID_ARG"):
        assert phrase in section, phrase


def test_bindings_and_symbol_list_name_the_entries(zg):
    assert set(NEW_ENTRIES) <= set(zg.ABI_SYMBOLS)
    for attr in ("fr_cube_root", "permutation_sigma"):
        assert callable(getattr(zg, attr))
    for attr in ("set_coset_generator", "coset_generator"):
        assert callable(getattr(zg.Ctx, attr))
    for attr in ("coset_generator", "export_key"):
        assert callable(getattr(zg.Prover, attr))
    assert [zg.KEY_FIXED_POLY, zg.KEY_SIGMA_POLY, zg.KEY_FIXED_COSET, zg.KEY_SIGMA_COSET, zg.KEY_L0, zg.KEY_L_LAST,
            zg.KEY_L_ACTIVE_ROW] == list(range(7))
