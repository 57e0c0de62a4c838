"""The device-resident dense surface exists (no GPU needed: dlsym, attribute
and header checks)."""
import os

import pytest

SYMBOLS = ["conflux_lu_set_matrix_device", "conflux_lu_get_factors_device",
           "conflux_lu_solve_device", "conflux_chol_solve_device",
           "conflux_lu_slogdet", "conflux_chol_logdet",
           "conflux_lu_logical_order"]


@pytest.mark.parametrize("name", SYMBOLS + ["conflux_lu_debug_get_input"])
def test_dense_symbol_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if undefined
    assert fn.argtypes, f"{name}: argtypes not declared in conflux_amd"


@pytest.mark.parametrize("name", ["set_matrix_device", "get_factors_device",
                                  "solve_device", "solve_cholesky_device",
                                  "slogdet", "logdet_cholesky"])
def test_engine_has_method(name):
    import conflux_amd
    assert callable(getattr(conflux_amd.Engine, name))


def test_engine_has_n_property():
    import conflux_amd
    assert isinstance(conflux_amd.Engine.n, property)


@pytest.mark.parametrize("name", SYMBOLS)
def test_header_declares(name):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include",
                            "conflux_lu.h")).read()
    assert f"int {name}(" in hdr


def test_dense_module_surface():
    from conflux_amd import dense
    for name in ("lu_factor", "cholesky_factor"):
        assert callable(getattr(dense, name))
    for name in ("solve", "solve_transposed", "slogdet", "rcond", "factors",
                 "close", "__enter__", "__exit__"):
        assert callable(getattr(dense.LU, name)), name
    for name in ("solve", "logdet", "rcond", "close"):
        assert callable(getattr(dense.Cholesky, name)), name


@pytest.mark.parametrize("n,v", [(1, 32), (63, 32), (64, 32), (127, 32),
                                 (128, 64), (255, 64), (256, 128),
                                 (1000, 256), (1024, 512), (16384, 512)])
def test_default_tile(n, v):
    """The largest of 512/256/128/64/32 with 2 v <= n, 32 below 64."""
    from conflux_amd import dense
    assert dense.default_v(n) == v
