"""The device validators shown WRONG factors: one element of the stored factor
is poked by 1.0, the residual is recomputed in numpy from the poked factors as
they read back, and conflux_lu_validate / conflux_chol_validate must agree to
1e-9 relative.  Both sides are fp64 sums over the same numbers (worst-case
accumulation error N^2 u = 3e-11 at N = 512, a thirtieth of the tolerance); a
validator that skipped the stripe, tile owner or triangle holding the poked
element would be off by orders of magnitude.  A poke of the strictly upper
part of a stored Cholesky factor must leave the validator's value bitwise
unchanged: consumers read tril only."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

# (N, v, Px, Py, Pz, real one-rank mode)
LU_CASES = [(256, 64, 1, 1, 1, False), (256, 64, 1, 1, 1, True),
            (512, 64, 2, 2, 1, False), (256, 64, 1, 1, 2, False)]
CHOL_CASES = [(256, 64, 1, 1, 1, False), (512, 64, 2, 2, 1, False)]


def corner_pokes(N, v, lower_only):
    p = [(0, 0), (N - 1, N - 1), (N - 1, 0), (v, v - 1)]
    return p if lower_only else p + [(0, N - 1)]


def owner_pokes(v, tiles):
    """One element inside each listed tile; on 2x2x1 tile (ti, tj) lives on
    rank (ti % 2, tj % 2)."""
    return [(ti * v + 3 + ti, tj * v + 5 + tj) for ti, tj in tiles]


# tiles owned by (0,0), (1,0), (0,1), (1,1); LU: two in L, two in U
LU_OWNER_TILES = [(4, 2), (3, 4), (4, 3), (5, 7)]
CHOL_OWNER_TILES = [(4, 2), (5, 2), (4, 3), (5, 3)]


def _params(cases, chol):
    out = []
    for case in cases:
        N, v, Px, Py = case[:4]
        pokes = corner_pokes(N, v, lower_only=chol)
        if (Px, Py) == (2, 2):
            tiles = CHOL_OWNER_TILES if chol else LU_OWNER_TILES
            assert sorted((ti % 2, tj % 2) for ti, tj in tiles) == \
                [(0, 0), (0, 1), (1, 0), (1, 1)]
            pokes = pokes + owner_pokes(v, tiles)
        out += [pytest.param(case, p, id=f"{N}-{v}-{Px}x{Py}x{case[4]}"
                             f"{'-real' if case[5] else ''}-{p[0]}_{p[1]}")
                for p in pokes]
    return out


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


_INPUT = {}


def _input(N, chol):
    if (N, chol) not in _INPUT:
        A = gen_matrix(N)
        if chol:
            A = 0.5 * (A + A.T) + 2.0 * N * np.eye(N)
        A.setflags(write=False)
        _INPUT[(N, chol)] = A
    return _INPUT[(N, chol)]


def _factored(eng, case, chol):
    N, v, Px, Py, Pz, real = case
    A = _input(N, chol)
    e = eng.Engine(N, v, Px, Py, Pz, rank=0, world=1) if real \
        else eng.Engine(N, v, Px, Py, Pz, rank=-1)
    e.store_factors(True)
    if real:
        e.set_matrix_local(A)
    else:
        e.set_matrix_global(A)
    if chol:
        e.factor_cholesky()
    else:
        e.factor()
    return e, A


def _read_F(e, real):
    return e.get_F_local() if real else e.get_F_global()


def _poke(eng, e, row, col, delta):
    rc = eng.lib().conflux_lu_debug_poke_factor(e._h, row, col, delta)
    assert rc == 0


@pytest.mark.parametrize("case,poke", _params(LU_CASES, chol=False))
def test_lu_validate_sees_a_poked_factor(eng, case, poke):
    N, real = case[0], case[5]
    e, A = _factored(eng, case, chol=False)
    with e:
        F0 = _read_F(e, real)
        _poke(eng, e, poke[0], poke[1], 1.0)
        F = _read_F(e, real)
        perm = e.get_perm()
        r_dev = e.validate()
    D = F - F0
    assert D[poke] == pytest.approx(1.0, abs=1e-12) and \
        np.count_nonzero(D) == 1, "the poke landed elsewhere"
    L = np.tril(F, -1) + np.eye(N)
    U = np.triu(F)
    r_np = np.linalg.norm(A[perm] - L @ U) / np.linalg.norm(A)
    print(f"VALIDATE lu {case} {poke} r_np={r_np:.6e} r_dev={r_dev:.6e} "
          f"rel={abs(r_dev - r_np) / r_np:.2e}")
    assert r_np > 1e-6
    assert abs(r_dev - r_np) <= 1e-9 * r_np


@pytest.mark.parametrize("case,poke", _params(CHOL_CASES, chol=True))
def test_chol_validate_sees_a_poked_factor(eng, case, poke):
    e, A = _factored(eng, case, chol=True)
    with e:
        F0 = _read_F(e, False)
        _poke(eng, e, poke[0], poke[1], 1.0)
        F = _read_F(e, False)
        r_dev = e.validate_cholesky()
    D = F - F0
    assert D[poke] == pytest.approx(1.0, abs=1e-12) and \
        np.count_nonzero(D) == 1, "the poke landed elsewhere"
    L = np.tril(F)
    r_np = np.linalg.norm(A - L @ L.T) / np.linalg.norm(A)
    print(f"VALIDATE chol {case} {poke} r_np={r_np:.6e} r_dev={r_dev:.6e} "
          f"rel={abs(r_dev - r_np) / r_np:.2e}")
    assert r_np > 1e-6
    assert abs(r_dev - r_np) <= 1e-9 * r_np


@pytest.mark.parametrize("case", CHOL_CASES,
                         ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}")
def test_chol_validate_ignores_the_upper_triangle(eng, case):
    N = case[0]
    vals = []
    for poked in (False, True):
        e, _ = _factored(eng, case, chol=True)   # a fresh engine each time
        with e:
            if poked:
                F0 = _read_F(e, False)
                _poke(eng, e, 0, N - 1, 1.0)
                D = _read_F(e, False) - F0
                assert D[0, N - 1] == pytest.approx(1.0, abs=1e-12) and \
                    np.count_nonzero(D) == 1
            vals.append(e.validate_cholesky())
            vals.append(e.validate_cholesky())   # and the same bits twice
    assert vals[0] < 1e-13
    bits = [np.float64(x).view(np.uint64) for x in vals]
    assert bits[0] == bits[1] == bits[2] == bits[3], vals


def test_poke_bad_arguments_are_refused(eng):
    N, v = 64, 8
    poke = eng.lib().conflux_lu_debug_poke_factor
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(gen_matrix(N))
        assert poke(e._h, 0, 0, 1.0) == -1      # nothing factored yet
        e.factor()
        for row, col in [(-1, 0), (0, -1), (N, 0), (0, N)]:
            assert poke(e._h, row, col, 1.0) == -1
        F0 = e.get_F_global()
        assert poke(e._h, 9, 17, 0.5) == 0
        D = e.get_F_global() - F0
        assert D[9, 17] == pytest.approx(0.5, abs=1e-12) and \
            np.count_nonzero(D) == 1
    assert poke(ctypes.c_void_p(), 0, 0, 1.0) == -1
