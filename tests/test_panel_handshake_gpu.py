"""Panel hand-off protocol tests (k_panel_factor's per-column handshake).

Per column every block publishes its candidate as two self-validating key
granules ((epoch<<32)|hi32 and (epoch<<32)|lo32 of the |value| bits) plus a
candidate record that also carries the row index; ties between blocks go to
the lower block index, which equals "smaller row wins" because blocks own
contiguous ascending row ranges.  These tests pin what that protocol must
keep: the LAPACK first-max pivot rule across block boundaries, block counts
above one wave's worth of pollers, all-zero columns, and rejection of stale
slots when panels of different heights reuse one sync struct.

Panel-level cases go through conflux_lu_debug_getrf.  The reference is
getrf_ref below: a plain unblocked numpy restatement of the kernel's
documented rule (first row with the largest |value| among rows c..n, swap,
multiply by the reciprocal of the pivot, rank-1 update).  Where LAPACK's
answer is unambiguous (no zero pivot) scipy's dgetrf is checked too; both
references were confirmed to agree on the pivots of every such input.  The
zero-column inputs are checked against the numpy restatement alone: LAPACK
reports a singular factor there and what it leaves in later columns is not
part of its contract.

NaN inputs are not tested: LAPACK's choice there is implementation-defined.
The key granules carry the full 64-bit pattern of the candidate value, so the
kernel's comparisons — and with them its behaviour on NaN — are unchanged by
construction.
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


def check_both_refs(eng, P0, tag):
    """Pivots bit-exact and factors <= TOL_F vs the numpy restatement AND
    LAPACK."""
    import scipy.linalg as la
    F, ipiv = gpu_getrf(eng, P0)
    Fr, pr = getrf_ref(P0)
    lu, pl, info = la.lapack.dgetrf(np.asfortranarray(P0))
    assert info == 0
    nst = len(pr)
    print(f"{tag}: max|F-ref|={np.abs(F - Fr).max():.3e} "
          f"max|F-lapack|={np.abs(F - lu).max():.3e}")
    assert np.array_equal(ipiv, pr), f"{tag}: pivots vs restatement"
    assert np.array_equal(ipiv, pl[:nst]), f"{tag}: pivots vs LAPACK"
    assert np.abs(F - Fr).max() <= TOL_F, f"{tag}: factors vs restatement"
    assert np.abs(F - lu).max() <= TOL_F, f"{tag}: factors vs LAPACK"
    return ipiv


# 2, 3 and 8 blocks of 256 rows, a ragged last block, two sub-panels at
# v = 64 (the epoch runs on from one launch into the next)
@pytest.mark.parametrize("n,v", [(257, 32), (600, 64), (2048, 64)])
def test_block_counts(eng, n, v):
    rng = np.random.default_rng(100 + n)
    check_both_refs(eng, 5 + rng.random((n, v)), f"n={n} v={v}")


def test_more_than_64_blocks(eng):
    """66 blocks in one launch: lanes 0 and 1 of the polling wave each poll
    two blocks."""
    rng = np.random.default_rng(66)
    check_both_refs(eng, 5 + rng.random((16643, 32)), "n=16643 v=32")


@pytest.mark.parametrize("rows,signs,expect", [
    ((40, 300, 700), (1.0, -1.0, 1.0), 40),   # blocks 0, 1 and 2
    ((300, 700), (-1.0, 1.0), 300),           # blocks 1 and 2 only
    ((260, 270), (1.0, -1.0), 260),           # both inside block 1
])
def test_cross_block_ties(eng, rows, signs, expect):
    """Equal maxima of |value| in column 0: the first row wins, across
    blocks and inside one.  Column 0 involves no arithmetic, so the
    expected pivot is exact."""
    n, v = 1024, 32
    rng = np.random.default_rng(7)
    P0 = rng.uniform(-1.0, 1.0, (n, v))
    for r, s in zip(rows, signs):
        P0[r, 0] = 2.0 * s
    ipiv = check_both_refs(eng, P0, f"ties {rows}")
    assert ipiv[0] == expect


@pytest.mark.parametrize("signed", [False, True])
def test_zero_column(eng, signed):
    """Column 5 identically zero (signed: -0.0 in the upper half, +0.0 in
    the lower): every |value| ties at zero, so pivot 5 is row 5.  Checked
    against the numpy restatement alone (see the module docstring)."""
    n, v = 512, 32
    rng = np.random.default_rng(5)
    P0 = rng.uniform(-1.0, 1.0, (n, v))
    P0[:, 5] = 0.0
    if signed:
        P0[:n // 2, 5] = -0.0
    F, ipiv = gpu_getrf(eng, P0)
    Fr, pr = getrf_ref(P0)
    assert ipiv[5] == 5
    assert not np.isnan(F[:, :5]).any()
    assert np.array_equal(ipiv, pr)
    print(f"zero column signed={signed}: "
          f"max|F-ref| cols 0..4 = {np.abs(F[:, :5] - Fr[:, :5]).max():.3e}")
    assert np.abs(F[:, :5] - Fr[:, :5]).max() <= TOL_F


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(1024, 128, 2, 2, 1),
                                          (1024, 64, 1, 1, 1)])
def test_stale_slots(eng, N, v, Px, Py, Pz):
    """Panels of shrinking height alternate with 2v-row tournament panels on
    one sync struct, over three factorizations: slots left by a taller panel
    or an earlier run carry an older epoch and must be rejected."""
    A = gen_matrix(N, 42)
    ref = lu_oracle(A, Params(N, v, Px, Py, Pz))
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        perms = []
        for _ in range(3):
            e.init_matrix(42)
            e.factor()
            perms.append(e.get_perm())
    assert np.array_equal(perms[0], perms[1])
    assert np.array_equal(perms[0], perms[2])
    assert np.array_equal(perms[0], ref["perm"])
