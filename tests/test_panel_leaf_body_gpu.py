"""The register leaf against k_panel_factor where a column body can go wrong.

k_panel_factor_reg holds a thread's row in registers and indexes it by the
column; its multiplier comes from the reciprocal of the pivot the polling
wave landed.  Whatever form that body takes, it must return k_panel_factor's
bits: every case factors in all three modes (lds, reg+R1, reg+R2) and
compares ipiv and the factors' 64-bit patterns exactly (NaN-aware: on the
uint64 views); where noted, mode 0 is also held to the numpy restatement of
the rule with test_panel_reg_gpu's tolerance.

Cases: every column index 0..31 with its pivot planted in row c itself, beside
it in wave 0 of block 0, in wave 1 of block 0 and in block 3 (every column in
every role, the 15/16 boundary, both swap cases); a column of denormals
(reciprocal Inf, multipliers Inf and NaN, then columns without any candidate);
a NaN and an Inf in the matrix; negative and tiny-but-normal pivots; exact
zeros under a negative pivot (factors -0.0, which later updates have to leave
alone); 66 blocks; two leaves with the glue between them.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_F = 1e-12

# (CONFLUX_PANEL_REG, CONFLUX_PANEL_PUBLISH)
MODES = [("lds", 0, 0), ("reg+R1", 1, 0), ("reg+R2", 1, 1)]


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def getrf_ref(P, trace=False):
    """Unblocked column-by-column partial-pivoting LU of an n x v panel.
    trace: also return, for every column c, the column as it stands when its
    pivot is chosen and the original row each current row came from."""
    A = np.array(P, dtype=np.float64)
    n, v = A.shape
    nst = min(n, v)
    ipiv = np.zeros(nst, dtype=np.int32)
    orig = np.arange(n)
    cols, origs = [], []
    for c in range(nst):
        if trace:
            cols.append(A[:, c].copy())
            origs.append(orig.copy())
        p = c + int(np.argmax(np.abs(A[c:, c])))  # argmax: first maximum
        ipiv[c] = p
        if p != c:
            A[[c, p], :] = A[[p, c], :]
            orig[[c, p]] = orig[[p, c]]
        if A[c, c] != 0.0:
            A[c + 1:, c] *= 1.0 / A[c, c]
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c, c + 1:])
    if trace:
        return A, ipiv, cols, origs
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
    """Factor P0 in every mode; assert ipiv and the factors' bit patterns are
    equal (NaN-aware: the comparison is on the uint64 views).  Returns mode
    0's (factors, ipiv)."""
    res = []
    for name, reg, pub in MODES:
        with modes(eng, reg, pub):
            res.append((name,) + gpu_getrf(eng, P0))
    _, F0, p0 = res[0]
    for name, F, p in res[1:]:
        nd = int(np.count_nonzero(F.view(np.uint64) != F0.view(np.uint64)))
        print(f"{tag}: {name} vs lds: bit patterns that differ = {nd}")
        assert np.array_equal(p, p0), f"{tag}: ipiv, {name} vs lds"
        assert nd == 0, f"{tag}: factor bit patterns, {name} vs lds"
    return F0, p0


def check(eng, P0, tag):
    """all_modes, then mode 0 against the restatement."""
    F0, p0 = all_modes(eng, P0, tag)
    Fr, pr = getrf_ref(P0)
    print(f"{tag}: lds max|F-ref| = {np.abs(F0 - Fr).max():.3e}")
    assert np.array_equal(p0, pr), f"{tag}: pivots vs restatement"
    assert np.abs(F0 - Fr).max() <= TOL_F, f"{tag}: factors vs restatement"
    return p0


@pytest.fixture(scope="module")
def base():
    """A 1024 x 32 uniform(-1, 1) panel and the trace of its factorization.
    Columns before c do not depend on column c, so the state in which column
    c's pivot is chosen is known for every c from this one run, whatever is
    planted in column c afterwards."""
    rng = np.random.default_rng(2024)
    P0 = rng.uniform(-1.0, 1.0, (1024, 32))
    _, _, cols, origs = getrf_ref(P0, trace=True)
    return P0, cols, origs


def plant(base, c0, pos, value, colscale=1.0):
    """base's panel with column c0 scaled by colscale and one entry changed
    so that, when column c0's pivot is chosen, the row at position pos holds
    `value` (up to rounding): the updated entry is the original one minus
    terms that do not depend on it."""
    P0, cols, origs = base
    P = P0.copy()
    P[:, c0] *= colscale
    P[origs[c0][pos], c0] += value - cols[c0][pos] * colscale
    return P


def column_scale(base, c0):
    """max(1, largest |entry| among column c0's candidates): uniform(-1, 1)
    entries have grown past 3 in this panel's later columns (4.6 at most), so
    a planted pivot is 3.0 times this, not 3.0, to be the pivot for sure."""
    _, cols, _ = base
    return max(1.0, float(np.abs(cols[c0][c0:]).max()))


# where column c0's pivot is planted: row c0 itself (no swap); another row of
# wave 0 of block 0 (below 32 for every c0 but the last); wave 1 of block 0;
# block 3
def placements(c0):
    return [c0, c0 + 1 if c0 < 31 else 33, 100, 800]


@pytest.mark.parametrize("where", [0, 1, 2, 3])
@pytest.mark.parametrize("c0", range(32))
def test_every_column_every_role(eng, base, c0, where):
    pos = placements(c0)[where]
    P = plant(base, c0, pos, 3.0 * column_scale(base, c0))
    ipiv = check(eng, P, f"column {c0} pivot planted at {pos}")
    assert ipiv[c0] == pos


@pytest.mark.parametrize("col", [0, 9, 16])
def test_denormal_column(eng, col):
    """One column's entries all below 1e-310 in magnitude: its pivot's
    reciprocal is Inf and the multipliers are Inf or NaN."""
    rng = np.random.default_rng(310 + col)
    P0 = rng.uniform(-1.0, 1.0, (512, 32))
    P0[:, col] *= 1e-310
    assert np.abs(P0[:, col]).max() < 1e-310
    all_modes(eng, P0, f"denormal column {col}")


@pytest.mark.parametrize("variant", ["below", "in_u"])
def test_nan_and_inf(eng, variant):
    """One NaN and one Inf that are not pivots where they stand.  below: both
    in rows below the triangle (the NaN's row turns NaN from column 10 on and
    is never a candidate again, its wave's other lanes stay finite; the Inf is
    picked up as column 20's pivot, reciprocal 0).  in_u: the Inf stands in
    row 0's column 20 and row 0 is column 0's pivot, so it enters the pivot
    row: column 20 turns Inf, everything behind it NaN, and the last columns
    have no candidate at all."""
    rng = np.random.default_rng(99)
    P0 = rng.uniform(-1.0, 1.0, (512, 32))
    P0[300, 10] = np.nan
    if variant == "below":
        P0[77, 20] = np.inf
    else:
        P0[0, 0] = 4.0
        P0[0, 20] = np.inf
    all_modes(eng, P0, f"NaN and Inf, {variant}")


@pytest.mark.parametrize("where", [0, 1, 2, 3])
@pytest.mark.parametrize("c0", [0, 15, 16, 31])
def test_negative_pivot(eng, base, c0, where):
    pos = placements(c0)[where]
    P = plant(base, c0, pos, -3.0 * column_scale(base, c0))
    ipiv = check(eng, P, f"column {c0} pivot -3.0 at {pos}")
    assert ipiv[c0] == pos


@pytest.mark.parametrize("where", [0, 1, 2, 3])
@pytest.mark.parametrize("c0", [0, 15, 16, 31])
def test_tiny_normal_pivot(eng, base, c0, where):
    """Column c0 scaled far down, its pivot planted as 1e-300: the reciprocal
    is 1e300 and every multiplier is an ordinary number."""
    pos = placements(c0)[where]
    P = plant(base, c0, pos, 1e-300, colscale=1e-301 / column_scale(base, c0))
    ipiv = check(eng, P, f"column {c0} pivot 1e-300 at {pos}")
    assert ipiv[c0] == pos


def test_negative_zero_factors(eng):
    """Exact zeros in column 0 under a negative pivot: those rows' factors
    are -0.0, and every later column's update has to leave that bit pattern
    as it is, for multipliers of either sign."""
    rng = np.random.default_rng(3)
    P0 = rng.uniform(-1.0, 1.0, (1024, 32))
    P0[::3, 0] = 0.0
    P0[5, 0] = -2.0
    F0, p0 = all_modes(eng, P0, "negative-zero factors")
    Fr, pr = getrf_ref(P0)
    assert np.array_equal(p0, pr)
    assert np.abs(F0 - Fr).max() <= TOL_F
    # the case is what it claims to be: a negative pivot, -0.0 factors
    assert Fr[0, 0] == -2.0
    neg_zero = np.uint64(1) << np.uint64(63)
    assert np.count_nonzero(F0.view(np.uint64)[32:, 0] == neg_zero) > 100


def test_many_blocks(eng):
    """66 blocks of 256 rows: the record layout on the polling wave's
    two-keys-per-lane path."""
    rng = np.random.default_rng(66)
    check(eng, 5 + rng.random((16643, 32)), "n=16643 v=32")


def test_two_leaves(eng):
    """Two leaves and a glue on one sync struct, the epoch running on."""
    rng = np.random.default_rng(664)
    check(eng, 5 + rng.random((600, 64)), "n=600 v=64")
