"""The refined-solve surface exists (no GPU needed: dlsym and attribute
checks)."""
import os

import pytest

SYMBOLS = ["conflux_lu_solve_refined", "conflux_chol_solve_refined",
           "conflux_lu_debug_residual_dd"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_refine_symbol_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if undefined
    assert fn.argtypes, f"{name}: argtypes not declared in conflux_amd"


def test_engine_has_refined_methods():
    import conflux_amd
    assert callable(getattr(conflux_amd.Engine, "solve_refined"))
    assert callable(getattr(conflux_amd.Engine, "solve_cholesky_refined"))


def test_header_declares_refined_solves():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include",
                            "conflux_lu.h")).read()
    assert "int conflux_lu_solve_refined(" in hdr
    assert "int conflux_chol_solve_refined(" in hdr
