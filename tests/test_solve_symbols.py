"""The solve surface exists (no GPU needed: dlsym and attribute checks)."""
import pytest

SYMBOLS = ["conflux_lu_solve", "conflux_chol_solve",
           "conflux_lu_debug_trsm_left", "conflux_lu_debug_update_skinny"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_solve_symbol_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if undefined
    assert fn.argtypes, f"{name}: argtypes not declared in conflux_amd"


def test_engine_has_solve_methods():
    import conflux_amd
    assert callable(getattr(conflux_amd.Engine, "solve"))
    assert callable(getattr(conflux_amd.Engine, "solve_cholesky"))


def test_header_declares_solves():
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include",
                            "conflux_lu.h")).read()
    assert "int conflux_lu_solve(" in hdr
    assert "int conflux_chol_solve(" in hdr
