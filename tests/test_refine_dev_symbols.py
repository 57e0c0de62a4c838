"""The transposed and device-resident refined solves exist (no GPU needed:
dlsym, attribute, signature and header checks)."""
import inspect
import os

import pytest

SYMBOLS = ["conflux_lu_solve_refined_trans",
           "conflux_lu_solve_refined_device",
           "conflux_chol_solve_refined_device",
           "conflux_lu_debug_residual_dd_t"]
NARGS = {"conflux_lu_solve_refined_trans": 8,
         "conflux_lu_solve_refined_device": 10,
         "conflux_chol_solve_refined_device": 9,
         "conflux_lu_debug_residual_dd_t": 8}


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if undefined
    assert fn.argtypes is not None, f"{name}: argtypes not declared"
    assert len(fn.argtypes) == NARGS[name]


def test_chunk_getter():
    """The row reduction is cut into fixed-length chunks, so the getter the
    GPU tests size their cases by is exported."""
    import conflux_amd
    fn = conflux_amd.lib().conflux_lu_debug_residual_t_chunk
    assert fn.argtypes is not None and len(fn.argtypes) == 0
    assert fn() >= 1  # a constant: no GPU involved


def test_engine_has_methods():
    import conflux_amd
    for m in ("solve_transposed_refined", "solve_refined_device",
              "solve_cholesky_refined_device"):
        assert callable(getattr(conflux_amd.Engine, m)), m
    sig = inspect.signature(conflux_amd.Engine.solve_transposed_refined)
    assert sig.parameters["max_iter"].default == 10
    assert sig.parameters["return_info"].default is False
    sig = inspect.signature(conflux_amd.Engine.solve_refined_device)
    assert list(sig.parameters)[1:] == ["dB", "ldb", "nrhs", "trans",
                                        "max_iter"]
    sig = inspect.signature(conflux_amd.Engine.solve_cholesky_refined_device)
    assert list(sig.parameters)[1:] == ["dB", "ldb", "nrhs", "max_iter"]


def test_dense_keywords():
    from conflux_amd import dense
    for fn in (dense.LU.solve, dense.LU.solve_transposed,
               dense.Cholesky.solve):
        p = inspect.signature(fn).parameters
        assert p["refine"].default is False, fn
        assert p["return_info"].default is False, fn
    assert "refine=True" in dense.__doc__ and "pivot=False" in dense.__doc__


def test_header_declares_entry_points():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include",
                            "conflux_lu.h")).read()
    assert "int conflux_lu_solve_refined_trans(" in hdr
    assert "int conflux_lu_solve_refined_device(" in hdr
    assert "int conflux_chol_solve_refined_device(" in hdr
