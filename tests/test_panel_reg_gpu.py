"""Register-resident panel leaf (k_panel_factor_reg) and its two hand-off forms.

Full 32-column leaves run a second leaf kernel that keeps a thread's row in
registers (CONFLUX_PANEL_REG / conflux_lu_debug_set_panel_reg) and publishes
the per-column payload either as sc1 stores + drain + key (R1,
CONFLUX_PANEL_PUBLISH=0) or as self-validating granules with no drain (R2,
CONFLUX_PANEL_PUBLISH=1).  Ragged leaves and mode 0 stay on k_panel_factor.
The arithmetic and the pivot rule are the same, so every mode must return
the SAME BITS: the comparisons between modes are exact (np.array_equal on
ipiv, on the factors and on the factors' 64-bit patterns).  The old kernel
does not offer R2, so three modes are compared.

Mode 0 alone is also held against the numpy restatement of the rule and
against LAPACK, with the handshake test's tolerance (the zero-column inputs
against the restatement alone, as there).

Shapes: a second block with a single row; two leaves with the glue between
them and the epoch running on; a register leaf followed by a ragged 16-column
leaf of the old kernel on one sync struct; panels where every row is a
diagonal row; pivots planted in row 0, beside row c in wave 0 of block 0, in
another wave of block 0 and in block 3; ties across blocks; a zero column;
more blocks than the polling wave has lanes.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import Params, gen_matrix, lu_oracle  # noqa: E402

TOL_F = 1e-12

# (CONFLUX_PANEL_REG, CONFLUX_PANEL_PUBLISH)
MODES = [("lds", 0, 0), ("reg+R1", 1, 0), ("reg+R2", 1, 1)]


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


class modes:
    """Set the two leaf switches; put the previous modes back on exit."""

    def __init__(self, eng, reg, publish):
        self.lib, self.reg, self.publish = eng.lib(), reg, publish

    def __enter__(self):
        self.prev_reg = self.lib.conflux_lu_debug_set_panel_reg(self.reg)
        self.prev_pub = self.lib.conflux_lu_debug_set_panel_publish(
            self.publish)
        return self

    def __exit__(self, *exc):
        self.lib.conflux_lu_debug_set_panel_reg(self.prev_reg)
        self.lib.conflux_lu_debug_set_panel_publish(self.prev_pub)
        return False


def all_modes(eng, P0, tag):
    """Factor P0 in every mode; assert the results are bitwise equal.
    Returns mode 0's (factors, ipiv)."""
    res = []
    for name, reg, pub in MODES:
        with modes(eng, reg, pub):
            res.append((name,) + gpu_getrf(eng, P0))
    _, F0, p0 = res[0]
    for name, F, p in res[1:]:
        nd = int(np.count_nonzero(F.view(np.uint64) != F0.view(np.uint64)))
        print(f"{tag}: {name} vs lds: bit patterns that differ = {nd}")
        assert np.array_equal(p, p0), f"{tag}: ipiv, {name} vs lds"
        assert np.array_equal(F, F0), f"{tag}: factors, {name} vs lds"
        assert np.array_equal(F.view(np.uint64), F0.view(np.uint64)), \
            f"{tag}: factor bit patterns, {name} vs lds"
    return F0, p0


def check(eng, P0, tag, lapack=True):
    F0, p0 = all_modes(eng, P0, tag)
    Fr, pr = getrf_ref(P0)
    print(f"{tag}: lds max|F-ref| = {np.abs(F0 - Fr).max():.3e}")
    assert np.array_equal(p0, pr), f"{tag}: pivots vs restatement"
    assert np.abs(F0 - Fr).max() <= TOL_F, f"{tag}: factors vs restatement"
    if lapack:
        import scipy.linalg as la
        lu, pl, info = la.lapack.dgetrf(np.asfortranarray(P0))
        assert info == 0
        print(f"{tag}: lds max|F-lapack| = {np.abs(F0 - lu).max():.3e}")
        assert np.array_equal(p0, pl[:len(pr)]), f"{tag}: pivots vs LAPACK"
        assert np.abs(F0 - lu).max() <= TOL_F, f"{tag}: factors vs LAPACK"
    return p0


def test_switches_return_previous_mode(eng):
    lib = eng.lib()
    for fn in (lib.conflux_lu_debug_set_panel_reg,
               lib.conflux_lu_debug_set_panel_publish):
        prev = fn(0)
        try:
            assert prev in (0, 1)
            assert fn(1) == 0
            assert fn(7) == 1  # nonzero = on
            assert fn(0) == 1
        finally:
            fn(prev)


# ragged block; two leaves; a register leaf then a ragged 16-column leaf of
# the old kernel; single-block panels with zero and one row below the triangle
@pytest.mark.parametrize("n,v", [(257, 32), (600, 64), (2048, 64), (600, 48),
                                 (32, 32), (33, 32)])
def test_shapes(eng, n, v):
    rng = np.random.default_rng(100 + n + v)
    check(eng, 5 + rng.random((n, v)), f"n={n} v={v}")


def test_many_blocks(eng):
    """66 blocks of 256 rows: lanes 0 and 1 of the polling wave poll two
    keys each (the register kernel uses 256-row blocks as well)."""
    rng = np.random.default_rng(66)
    check(eng, 5 + rng.random((16643, 32)), "n=16643 v=32")


# row 0 itself (no swap); beside row c in wave 0 of block 0; another wave of
# block 0; block 3.  Later columns' pivots fall where the random data puts
# them.
@pytest.mark.parametrize("row", [0, 5, 100, 800])
def test_placed_pivot(eng, row):
    rng = np.random.default_rng(17)
    P0 = rng.uniform(-1.0, 1.0, (1024, 32))
    P0[row, 0] = 3.0
    ipiv = check(eng, P0, f"pivot planted in row {row}")
    assert ipiv[0] == row


@pytest.mark.parametrize("rows,signs,expect", [
    ((40, 300, 700), (1.0, -1.0, 1.0), 40),   # blocks 0, 1 and 2
    ((300, 700), (-1.0, 1.0), 300),           # blocks 1 and 2 only
    ((260, 270), (1.0, -1.0), 260),           # both inside block 1
])
def test_cross_block_ties(eng, rows, signs, expect):
    rng = np.random.default_rng(7)
    P0 = rng.uniform(-1.0, 1.0, (1024, 32))
    for r, s in zip(rows, signs):
        P0[r, 0] = 2.0 * s
    ipiv = check(eng, P0, f"ties {rows}")
    assert ipiv[0] == expect


@pytest.mark.parametrize("signed", [False, True])
def test_zero_column(eng, signed):
    """Column 5 identically zero (signed: -0.0 in the upper half): the
    zero-pivot path.  Mode 0 against the restatement on columns 0..4 as in
    the handshake test; the modes against each other on everything."""
    n, v = 512, 32
    rng = np.random.default_rng(5)
    P0 = rng.uniform(-1.0, 1.0, (n, v))
    P0[:, 5] = 0.0
    if signed:
        P0[:n // 2, 5] = -0.0
    F0, p0 = all_modes(eng, P0, f"zero column signed={signed}")
    Fr, pr = getrf_ref(P0)
    assert p0[5] == 5
    assert not np.isnan(F0[:, :5]).any()
    assert np.array_equal(p0, pr)
    assert np.abs(F0[:, :5] - Fr[:, :5]).max() <= TOL_F


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(1024, 64, 1, 1, 1),
                                          (1024, 128, 2, 2, 1)])
def test_engine_alternating_modes(eng, N, v, Px, Py, Pz):
    """Three factorizations on one engine, the mode changing in between:
    slots left by one mode meet the other's epochs on the same sync
    struct."""
    lib = eng.lib()
    A = gen_matrix(N, 42)
    ref = lu_oracle(A, Params(N, v, Px, Py, Pz))
    prev_reg = lib.conflux_lu_debug_set_panel_reg(1)
    prev_pub = lib.conflux_lu_debug_set_panel_publish(1)
    perms = []
    try:
        with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
            for reg, pub in [(1, 1), (0, 0), (1, 0), (1, 1)]:
                lib.conflux_lu_debug_set_panel_reg(reg)
                lib.conflux_lu_debug_set_panel_publish(pub)
                e.init_matrix(42)
                e.factor()
                perms.append(e.get_perm())
    finally:
        lib.conflux_lu_debug_set_panel_reg(prev_reg)
        lib.conflux_lu_debug_set_panel_publish(prev_pub)
    for p in perms[1:]:
        assert np.array_equal(perms[0], p)
    assert np.array_equal(perms[0], ref["perm"])


@pytest.mark.parametrize("reg,pub", [(0, 0), (1, 0), (1, 1)])
def test_instrumented_build(eng, reg, pub):
    """The instrumented instantiation returns the same bits and all four
    phase totals are non-zero."""
    lib = eng.lib()
    rng = np.random.default_rng(600)
    P0 = 5 + rng.random((600, 64))
    stats = np.zeros(9, dtype=np.uint64)
    with modes(eng, reg, pub):
        F0, p0 = gpu_getrf(eng, P0)
        prev = lib.conflux_lu_debug_set_panel_phase_stats(1)
        try:
            lib.conflux_lu_debug_panel_phase_stats(
                stats.ctypes.data_as(ctypes.c_void_p))  # reset
            F1, p1 = gpu_getrf(eng, P0)
            assert lib.conflux_lu_debug_panel_phase_stats(
                stats.ctypes.data_as(ctypes.c_void_p)) == 0
        finally:
            lib.conflux_lu_debug_set_panel_phase_stats(prev)
    print(f"reg={reg} publish={pub}: phase cycles {stats.tolist()}")
    assert np.array_equal(p0, p1)
    assert np.array_equal(F0.view(np.uint64), F1.view(np.uint64))
    assert stats[8] == 64
    assert (stats[:4] > 0).all() and (stats[4:8] > 0).all()
