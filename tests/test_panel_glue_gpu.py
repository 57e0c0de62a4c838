"""Fused inter-leaf glue of factor_panel (k_panel_glue_prep / _update).

After each 32-column leaf of a panel the engine permutes the leaf's rows over
the other columns, solves the 32-row U block right of the leaf and applies
the rank-32 update below it.  The default path does that in two purpose-built
launches; CONFLUX_PANEL_GLUE=0 (or conflux_lu_debug_set_panel_glue(0)) keeps
the four-launch chain it replaces (gather, scatter, 32-wide solve, K=32
GEMM).  The fused kernels use the same recurrence and the same MFMA k order,
so the two paths must agree BIT FOR BIT: every comparison between them here
is np.array_equal, never a tolerance.

Panel-level cases go through conflux_lu_debug_getrf.  Where a reference
besides the other path is needed it is getrf_ref: a plain unblocked numpy
restatement of the kernel's documented rule (first row with the largest
|value| among rows c..n, swap, multiply by the reciprocal of the pivot,
rank-1 update); pivots must be exact and factors within TOL_F, the bound the
panel hand-off tests use.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import Params, gen_matrix, lu_oracle  # noqa: E402

TOL_F = 1e-12


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def getrf_ref(P):
    """Unblocked column-by-column partial-pivoting LU of an n x v panel."""
    A = np.array(P, dtype=np.float64)
    n, v = A.shape
    nst = min(n, v)
    ipiv = np.zeros(nst, dtype=np.int32)
    for c in range(nst):
        p = c + int(np.argmax(np.abs(A[c:, c])))  # argmax: first maximum
        ipiv[c] = p
        if p != c:
            A[[c, p], :] = A[[p, c], :]
        if A[c, c] != 0.0:
            A[c + 1:, c] *= 1.0 / A[c, c]
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c, c + 1:])
    return A, ipiv


def gpu_getrf(eng, P0):
    n, v = P0.shape
    P1 = np.ascontiguousarray(P0).copy()  # factors in place
    ipiv = np.zeros(v, dtype=np.int32)
    rc = eng.lib().conflux_lu_debug_getrf(
        n, v, P1.ctypes.data_as(ctypes.c_void_p),
        ipiv.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return P1, ipiv[:min(n, v)]


def getrf_both(eng, P0):
    """Factor P0 on the four-launch chain (mode 0) and on the fused pair
    (mode 1); the process-wide mode is put back afterwards."""
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_panel_glue(0)
    try:
        F0, p0 = gpu_getrf(eng, P0)
        assert lib.conflux_lu_debug_set_panel_glue(1) == 0
        F1, p1 = gpu_getrf(eng, P0)
    finally:
        lib.conflux_lu_debug_set_panel_glue(prev)
    return F0, p0, F1, p1


def assert_bitwise(F0, p0, F1, p1, tag):
    ndiff = int(np.count_nonzero(F0 != F1))
    print(f"{tag}: elements that differ between the paths = {ndiff}, "
          f"max|F1-F0| = {np.abs(F1 - F0).max():.3e}")
    assert not np.isnan(F0).any() and not np.isnan(F1).any()
    assert np.array_equal(p0, p1), f"{tag}: ipiv differs between the paths"
    assert np.array_equal(F0, F1), f"{tag}: factors differ between the paths"


def test_switch_returns_previous_mode(eng):
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_panel_glue(0)
    try:
        assert prev in (0, 1)
        assert lib.conflux_lu_debug_set_panel_glue(1) == 0
        assert lib.conflux_lu_debug_set_panel_glue(7) == 1  # nonzero = fused
        assert lib.conflux_lu_debug_set_panel_glue(0) == 1
    finally:
        lib.conflux_lu_debug_set_panel_glue(prev)


# (65, 64): one glue step whose update has a single row
# (40, 64): 8 update rows, then a ragged nb = 8 leaf that falls back
# (600, 64): ragged row tiles
# (2048, 128): four leaves: left columns (jb > 0), shrinking right widths
# (1024, 512): the bench's v, 15 glue steps of widths 480..32; also the
#              tournament's 2v-row shape
# (16643, 32): no glue at all; the switch must be a no-op
@pytest.mark.parametrize("n,v", [(65, 64), (40, 64), (600, 64), (2048, 128),
                                 (1024, 512), (16643, 32)])
def test_bitwise_ab(eng, n, v):
    rng = np.random.default_rng(400 + n + v)
    P0 = 5 + rng.random((n, v))
    F0, p0, F1, p1 = getrf_both(eng, P0)
    assert_bitwise(F0, p0, F1, p1, f"n={n} v={v}")


def check_corner(eng, P0, tag):
    Fr, pr = getrf_ref(P0)
    F0, p0, F1, p1 = getrf_both(eng, P0)
    print(f"{tag}: max|F0-ref| = {np.abs(F0 - Fr).max():.3e} "
          f"max|F1-ref| = {np.abs(F1 - Fr).max():.3e}")
    assert_bitwise(F0, p0, F1, p1, tag)
    assert np.array_equal(p1, pr), f"{tag}: pivots vs restatement"
    assert np.abs(F1 - Fr).max() <= TOL_F, f"{tag}: factors vs restatement"
    assert np.abs(F0 - Fr).max() <= TOL_F, f"{tag}: chain vs restatement"
    return pr


def test_no_row_moves(eng):
    """Diagonally dominant panel: every pivot is the diagonal row, so each
    leaf's swap map is identity entries plus the padding that repeats
    entry 0."""
    n, v = 1024, 128
    rng = np.random.default_rng(11)
    P0 = rng.uniform(-1.0, 1.0, (n, v))
    P0[np.arange(v), np.arange(v)] = 10.0
    pr = check_corner(eng, P0, "diagonally dominant")
    assert np.array_equal(pr, np.arange(v))


def test_pivots_from_the_bottom(eng):
    """Every pivot comes from the last 128 rows, so every leaf has 32
    overflow entries whose rows lie in other row tiles than the leaf."""
    n, v = 1024, 128
    rng = np.random.default_rng(12)
    P0 = rng.uniform(-1.0, 1.0, (n, v))
    P0[n - v:, :] = 100.0 * np.eye(v)[::-1] + rng.uniform(-0.01, 0.01, (v, v))
    _, pr = getrf_ref(P0)
    assert (pr >= n - v).all()  # the construction, before the GPU is involved
    check_corner(eng, P0, "pivots from the bottom")


_ORACLE = {}


def oracle_perm(N, v, Px, Py, Pz):
    key = (N, v, Px, Py, Pz)
    if key not in _ORACLE:
        _ORACLE[key] = lu_oracle(gen_matrix(N, 42),
                                 Params(N, v, Px, Py, Pz))["perm"]
    return _ORACLE[key]


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(1024, 128, 2, 2, 1),
                                          (1024, 64, 1, 1, 1)])
def test_engine_perm(eng, N, v, Px, Py, Pz):
    """Whole factorizations (panels of shrinking height alternating with the
    tournament's 2v-row panels), once per glue mode: same permutation, and
    the oracle's."""
    lib = eng.lib()
    perms = []
    prev = lib.conflux_lu_debug_set_panel_glue(0)
    try:
        for mode in (0, 1):
            lib.conflux_lu_debug_set_panel_glue(mode)
            with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
                e.init_matrix(42)
                e.factor()
                perms.append(e.get_perm())
    finally:
        lib.conflux_lu_debug_set_panel_glue(prev)
    assert np.array_equal(perms[0], perms[1])
    assert np.array_equal(perms[1], oracle_perm(N, v, Px, Py, Pz))
