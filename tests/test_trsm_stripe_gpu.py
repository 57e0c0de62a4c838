"""GPU tests of the stripe-resident fused panel solves.

After each panel the engine solves A10 <- A10 U^-1 (right solve; Cholesky
runs the same kernel transposed, A10 <- A10 L^-T) and A01 <- L^-1 A01 (left
solve).  The default kernels keep a block's 32-wide stripe of X in LDS for
the whole v x v triangle; CONFLUX_TRSM_STRIPE=0 (or
conflux_lu_debug_set_trsm_stripe(0)) keeps the kernels they replace, which
stream every solved panel through LDS again for each diagonal block.  Both
use the same left-looking recurrence, the same MFMA k order and the same
diagonal solve, and rows (right) / columns (left) of X are independent, so the
two modes must agree BIT FOR BIT: every comparison between them here is
np.array_equal.  The new mode is also checked against a numpy solve at the
bound tests/test_engine_gpu.py uses for the fused solves (max |err| < 1e-12).

The triangles are well conditioned (unit lower / upper with |diagonal| in
[1, 2], off-diagonal row sums <= 0.5) so ||T^-1||inf <= 2 at every v and the
1e-12 bound holds at v = 512 as it does at v = 64.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import Params, gen_matrix, lu_oracle  # noqa: E402

TOL = 1e-12  # tests/test_engine_gpu.py: test_trsm_right_upper / _left_lower_unit

# no update iteration; one; the first toggle of the prefetch buffer; the
# bench tile (the LDS limit of the resident stripe)
VS = [32, 64, 96, 512]


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sizes(eng):
    W = eng.lib().conflux_lu_debug_trsm_stripe_width()
    assert W > 1
    return [1, W - 1, W, W + 1, 3 * W + 5]


def upper_tri(rng, v):
    U = np.triu(rng.uniform(-1, 1, (v, v)), 1) * (0.5 / v)
    d = rng.uniform(1, 2, v) * rng.choice([-1.0, 1.0], v)
    return U + np.diag(d)


def unit_lower_tri(rng, v):
    return np.tril(rng.uniform(-1, 1, (v, v)), -1) * (0.5 / v) + np.eye(v)


def solve_ld(eng, side_right, trans, v, n, ldx, off, T, X):
    X1 = np.ascontiguousarray(X).copy()
    rc = eng.lib().conflux_lu_debug_trsm_ld(side_right, trans, v, n, ldx, off,
                                            _p(np.ascontiguousarray(T)),
                                            _p(X1))
    assert rc == 0
    return X1


def both_modes(eng, *args):
    """Run one debug solve on the streaming kernels (mode 0) and on the
    stripe-resident ones (mode 1); the process-wide mode is put back."""
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_trsm_stripe(0)
    try:
        X0 = solve_ld(eng, *args)
        assert lib.conflux_lu_debug_set_trsm_stripe(1) == 0
        X1 = solve_ld(eng, *args)
    finally:
        lib.conflux_lu_debug_set_trsm_stripe(prev)
    return X0, X1


def test_switch_returns_previous_mode(eng):
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_trsm_stripe(0)
    try:
        assert prev in (0, 1)
        assert lib.conflux_lu_debug_set_trsm_stripe(1) == 0
        assert lib.conflux_lu_debug_set_trsm_stripe(7) == 1  # nonzero = stripe
        assert lib.conflux_lu_debug_set_trsm_stripe(0) == 1
    finally:
        lib.conflux_lu_debug_set_trsm_stripe(prev)


@pytest.mark.parametrize("v", VS)
def test_right_solve_bitwise_and_numpy(eng, v):
    """X * U^-1 (trans=0) and X * L^-T (trans=1) for M rows around the
    stripe width, X tight (ldx = v, the engine's call) and inside a wider
    array (ldx > v, column offset)."""
    rng = np.random.default_rng(100 + v)
    U = upper_tri(rng, v)
    for M in sizes(eng):
        for (ldx, off) in [(v, 0), (v + 7, 3)]:
            X = rng.standard_normal((M, ldx))
            ref = X[:, off:off + v] @ np.linalg.inv(U)
            outs = []
            for trans, T in [(0, U), (1, U.T)]:
                X0, X1 = both_modes(eng, 1, trans, v, M, ldx, off, T, X)
                tag = f"right v={v} M={M} ldx={ldx} off={off} trans={trans}"
                err = np.abs(X1[:, off:off + v] - ref).max()
                print(f"{tag}: differ={np.count_nonzero(X0 != X1)} "
                      f"err={err:.3e}")
                assert np.isfinite(X1).all(), tag
                assert np.array_equal(X0, X1), tag
                # nothing outside the window is written
                keep = np.ones(ldx, bool)
                keep[off:off + v] = False
                assert np.array_equal(X1[:, keep], X[:, keep]), tag
                assert err < TOL, f"{tag}: err={err}"
                outs.append(X1)
            # the transposed read of the same triangle is the same solve
            assert np.array_equal(outs[0], outs[1]), f"v={v} M={M} trans"


@pytest.mark.parametrize("v", VS)
def test_left_solve_bitwise_and_numpy(eng, v):
    """L^-1 * X for N columns around the stripe width, X tight (ldx = N) and
    as a window of a wider array (ldx > N, non-zero column offset: the
    engine's A01 call)."""
    rng = np.random.default_rng(200 + v)
    L = unit_lower_tri(rng, v)
    for N in sizes(eng):
        for (ldx, off) in [(N, 0), (N + 13, 5)]:
            X = rng.standard_normal((v, ldx))
            ref = np.linalg.solve(L, X[:, off:off + N])
            X0, X1 = both_modes(eng, 0, 0, v, N, ldx, off, L, X)
            tag = f"left v={v} N={N} ldx={ldx} off={off}"
            err = np.abs(X1[:, off:off + N] - ref).max()
            print(f"{tag}: differ={np.count_nonzero(X0 != X1)} err={err:.3e}")
            assert np.isfinite(X1).all(), tag
            assert np.array_equal(X0, X1), tag
            keep = np.ones(ldx, bool)
            keep[off:off + N] = False
            assert np.array_equal(X1[:, keep], X[:, keep]), tag
            assert err < TOL, f"{tag}: err={err}"


# ---------------- engine level: both modes, factors and pivots bitwise ------

def _spd(N):
    rng = np.random.default_rng(7)
    B = rng.standard_normal((N, N))
    return B @ B.T / N + np.eye(N) * 4


def factor_sim(eng, A, v, Px, Py, Pz, chol=False):
    N = A.shape[0]
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        if chol:
            e.factor_cholesky()
            return None, e.get_F_global()
        e.factor()
        return e.get_perm(), e.get_F_global()


def factor_single_rank(eng, A, v):
    """1x1x1 as ONE RANK (not the simulation): the lookahead order with the
    left solve on its own stream — the path the benchmark times."""
    N = A.shape[0]
    with eng.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
        e.store_factors(True)
        e.set_matrix_local(A)
        e.factor()
        return e.get_perm(), e.get_F_local()


def in_both_modes(eng, fn):
    lib = eng.lib()
    out = []
    prev = lib.conflux_lu_debug_set_trsm_stripe(0)
    try:
        for mode in (0, 1):
            lib.conflux_lu_debug_set_trsm_stripe(mode)
            out.append(fn())
    finally:
        lib.conflux_lu_debug_set_trsm_stripe(prev)
    return out


def assert_same(r0, r1, tag):
    (p0, F0), (p1, F1) = r0, r1
    print(f"{tag}: factor elements that differ = "
          f"{np.count_nonzero(F0 != F1)}")
    assert np.isfinite(F1).all(), tag
    if p0 is not None:
        assert np.array_equal(p0, p1), f"{tag}: perm"
    assert np.array_equal(F0, F1), f"{tag}: factors"


@pytest.mark.parametrize("Px,Py,Pz", [(1, 1, 1), (2, 2, 1), (1, 1, 2)])
def test_engine_lu_bitwise_sim(eng, Px, Py, Pz):
    N, v = 1024, 128
    A = gen_matrix(N)
    r0, r1 = in_both_modes(eng, lambda: factor_sim(eng, A, v, Px, Py, Pz))
    assert_same(r0, r1, f"LU N={N} v={v} sim {Px}x{Py}x{Pz}")
    if (Px, Py, Pz) == (1, 1, 1):  # pivots also match the oracle exactly
        ref = lu_oracle(A, Params(N, v, 1, 1, 1))
        assert np.array_equal(r1[0], ref["perm"])


@pytest.mark.parametrize("N,v", [(1024, 128), (2048, 512)])
def test_engine_lu_bitwise_single_rank(eng, N, v):
    A = gen_matrix(N)
    r0, r1 = in_both_modes(eng, lambda: factor_single_rank(eng, A, v))
    assert_same(r0, r1, f"LU N={N} v={v} one rank")


def test_engine_cholesky_bitwise(eng):
    N, v = 1024, 128
    A = _spd(N)
    r0, r1 = in_both_modes(
        eng, lambda: factor_sim(eng, A, v, 1, 1, 1, chol=True))
    assert_same(r0, r1, f"Cholesky N={N} v={v}")
    L = np.tril(r1[1])
    assert np.linalg.norm(A - L @ L.T) / np.linalg.norm(A) < 1e-14
