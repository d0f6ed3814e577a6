"""The DILU smoother's inspection entries at the C-ABI boundary (no GPU needed): declared in include/dfmi.h,
exported by the built library, bound by the Python mirror; the option is in the option table."""
import os
import re

from conftest import ROOT

ENTRIES = ("dfmi_amg_smoother_info", "dfmi_amg_apply")


def test_header_declares_the_inspection_entries():
    txt = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*dfmi_ctx\s*\*" % s, code), s
    assert "MULTICOLOR_DILU" in txt   # the option comment cites the amgxpOptions line


def test_library_exports_and_binding_mirrors_them():
    from dfmi import lib
    L = lib.load()
    for s in ENTRIES:
        assert hasattr(L, s), s
        assert s in lib.exported_symbols(), s
    assert hasattr(lib.Context, "amg_smoother_info") and hasattr(lib.Context, "amg_apply")


def test_option_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`amg.smoother`" in doc and "MULTICOLOR_DILU" in doc
    ctx_h = open(os.path.join(ROOT, "deepflame-dev_amd", "csrc", "dfmi_ctx.h")).read()
    assert '{"amg.smoother", 0}' in ctx_h   # the default stays weighted Jacobi
