"""The transposed-solve and condition-estimate surface exists (no GPU needed:
dlsym and attribute checks)."""
import os

import pytest

SYMBOLS = ["conflux_lu_solve_trans", "conflux_lu_rcond", "conflux_chol_rcond",
           "conflux_lu_debug_trsm_left_trans",
           "conflux_lu_debug_update_skinny_t"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_trans_rcond_symbol_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if undefined
    assert fn.argtypes, f"{name}: argtypes not declared in conflux_amd"


@pytest.mark.parametrize("name", ["solve_transposed", "rcond",
                                  "rcond_cholesky"])
def test_engine_has_method(name):
    import conflux_amd
    assert callable(getattr(conflux_amd.Engine, name))


@pytest.mark.parametrize("name", ["conflux_lu_solve_trans",
                                  "conflux_lu_rcond", "conflux_chol_rcond"])
def test_header_declares(name):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include",
                            "conflux_lu.h")).read()
    assert f"int {name}(" in hdr
