"""GPU tests of the transposed and the device-resident refined solves
(conflux_lu_solve_refined_trans, conflux_lu_solve_refined_device,
conflux_chol_solve_refined_device, and refine= in conflux_amd.dense): the
transposed doubled-precision residual kernel against the exactly rounded
residual, exact recovery and the no-pivot rescue for A^T X = B, device B
against host B, the logical order n < N_padded, slack and guards.

All tests run on ONE MI355X; multi-rank grids use the engine's
single-process simulation mode (rank=-1).  The helpers _two_prod,
_exact_residual, _berr_host and _int_system are test_refine_gpu.py's methods.
"""
import ctypes
import math

import numpy as np
import pytest
# torch before the engine's library is loaded anywhere in this process (see
# test_dense_gpu.py and conflux_amd/dense.py)
import torch as _torch  # noqa: F401

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

import _hp_ref as hp  # noqa: E402

EARG = -1
U = 2.0 ** -53
GRIDS = [(1, 1, 1), (2, 2, 1)]


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


@pytest.fixture(scope="module")
def torch():
    return _torch


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------- kernel: transposed doubled-precision residual -------------

def _two_prod(a, x):
    """Dekker/Veltkamp: p + e == a * x exactly (no FMA needed)."""
    p = a * x
    c = 134217729.0  # 2^27 + 1
    t = c * a
    ah = t - (t - a)
    al = a - ah
    t = c * x
    xh = t - (t - x)
    xl = x - xh
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    return p, e


def _exact_residual(A, X, B):
    """fl(B - A X): every product split into p + e exactly, then one
    correctly rounded sum (math.fsum) per entry."""
    M, n = A.shape[0], X.shape[1]
    R = np.empty((M, n))
    for j in range(n):
        p, e = _two_prod(A, X[:, j][None, :])
        T = np.concatenate([B[:, j:j + 1], -p, -e], axis=1)
        for i in range(M):
            R[i, j] = math.fsum(T[i])
    return R


def _residual_bar_t(A, X, B, Rex):
    """The bar of test_refine_gpu.py with the reduction length M."""
    M = A.shape[0]
    return 2 * U * np.abs(Rex) + \
        2 * (M + 2) ** 2 * U * U * (np.abs(A.T) @ np.abs(X) + np.abs(B))


def _gpu_residual_t(eng, A, X, B, lda, Rbuf=None):
    """R = B - A^T X through the debug entry.  Padding columns of A and a
    two-row tail behind A and X hold NaN: neither may be read."""
    M, K = A.shape
    nrhs = X.shape[1]
    Ad = np.full((M + 2, lda), np.nan)
    Ad[:M, :K] = A
    Xd = np.full((M + 2, nrhs), np.nan)
    Xd[:M] = X
    R = np.full((K, nrhs), np.nan) if Rbuf is None else Rbuf
    rc = eng.lib().conflux_lu_debug_residual_dd_t(
        M, K, nrhs, lda, _p(Ad), _p(Xd), _p(np.ascontiguousarray(B)), _p(R))
    assert rc == 0
    return R


def _group_width(eng):
    return eng.lib().conflux_lu_debug_residual_group_width()


def _chunk(eng):
    return eng.lib().conflux_lu_debug_residual_t_chunk()


# C = the chunk the row reduction is cut into
RES_M = ["1", "15", "17", "300", "1000", "C-1", "C", "C+1", "2C+1"]
RES_K = [1, 63, 64, 65, 130]
RES_NRHS = ["1", "3", "G", "G+1", "17"]  # G = the kernel's column group


@pytest.mark.parametrize("nrhs_tag", RES_NRHS)
@pytest.mark.parametrize("M_tag", RES_M)
def test_residual_dd_t_exact(eng, M_tag, nrhs_tag):
    """The transposed residual vs the exactly rounded one, elementwise
        |R - R_exact| <= 2u|R_exact| + 2(M+2)^2 u^2 (|A^T||X| + |B|):
    test_refine_gpu.py's bar with the reduction length M in place of K; it
    comes from the dd arithmetic, not from any output.  B = fl(A^T X), so
    the true residual is pure rounding error: at M = 1000 numpy's
    working-precision B - A.T @ X misses the bar on more than half the
    entries (asserted).  One reference at K = 130 serves every K (columns of
    A are independent); every M needs its own.  lda = K + 3 and odd K reach
    the scalar path."""
    G, C = _group_width(eng), _chunk(eng)
    assert G >= 1 and C >= 1
    nrhs = {"G": G, "G+1": G + 1}.get(nrhs_tag) or int(nrhs_tag)
    M = {"C-1": C - 1, "C": C, "C+1": C + 1,
         "2C+1": 2 * C + 1}.get(M_tag) or int(M_tag)
    if M < 1:
        M = 1
    rng = np.random.default_rng(1000 * M + nrhs)
    A = rng.standard_normal((M, max(RES_K)))
    X = rng.standard_normal((M, nrhs))
    B = A.T @ X
    Rex = _exact_residual(np.ascontiguousarray(A.T), X, B)
    bar = _residual_bar_t(A, X, B, Rex)
    if M == 1000:
        miss = np.abs((B - A.T @ X) - Rex) > bar
        print(f"numpy residual misses the bar on {miss.mean():.0%}")
        assert miss.mean() > 0.5
    for K in RES_K:
        for lda in (K, K + 3):
            R = _gpu_residual_t(eng, A[:, :K], X, B[:K], lda)
            assert np.isfinite(R).all(), \
                f"NaN leaked from the padding: M={M} K={K} lda={lda}"
            excess = (np.abs(R - Rex[:K]) / bar[:K]).max()
            print(f"resid_t M={M} K={K} nrhs={nrhs} lda={lda}: "
                  f"max err/bar={excess:.3g}")
            assert (np.abs(R - Rex[:K]) <= bar[:K]).all(), \
                f"M={M} K={K} nrhs={nrhs} lda={lda}: err/bar={excess}"


def _arange_case(nrhs):
    M, K = 200, 70
    A = np.arange(M * K, dtype=np.float64).reshape(M, K) / 100
    X = (np.arange(M * nrhs, dtype=np.float64).reshape(M, nrhs) ** 1.5) / 1000
    B = np.sqrt(np.arange(K * nrhs, dtype=np.float64).reshape(K, nrhs))
    return A, X, B


@pytest.mark.parametrize("nrhs", [3, 17])
def test_residual_dd_t_transpose_detecting(eng, nrhs):
    # asymmetric A, X and B catch a missing transpose, a row permutation
    # that A and X disagree on, or columns landing in the wrong group
    A, X, B = _arange_case(nrhs)
    Rex = _exact_residual(np.ascontiguousarray(A.T), X, B)
    R = _gpu_residual_t(eng, A, X, B, A.shape[1])
    assert (np.abs(R - Rex) <= _residual_bar_t(A, X, B, Rex)).all()


@pytest.mark.parametrize("nrhs", [3, 17])
def test_residual_dd_t_deterministic_and_framed(eng, nrhs):
    """Two calls agree bitwise (the merge order is fixed by indices), a
    column's bits do not depend on the group it lands in, and nothing is
    written outside R's K x nrhs."""
    C = _chunk(eng)
    M, K = 2 * C + 37, 130
    rng = np.random.default_rng(nrhs)
    A = rng.standard_normal((M, K))
    X = rng.standard_normal((M, nrhs))
    B = A.T @ X
    R1 = _gpu_residual_t(eng, A, X, B, K)
    R2 = _gpu_residual_t(eng, A, X, B, K)
    assert hp.bits_equal(R1, R2)
    # odd lda: the scalar path loads the same values
    assert hp.bits_equal(R1, _gpu_residual_t(eng, A, X, B, K + 3))
    # column 2 alone (its own group of one) has the bits it had in the group
    Rc = _gpu_residual_t(eng, A, np.ascontiguousarray(X[:, 2:3]),
                         np.ascontiguousarray(B[:, 2:3]), K)
    assert hp.bits_equal(R1[:, 2:3], Rc)
    buf = hp.canvas(K + 3, nrhs)
    _gpu_residual_t(eng, A, X, B, K, Rbuf=buf)
    assert hp.frame_intact(buf, K, nrhs)
    assert hp.bits_equal(buf[:K], R1)


def test_residual_dd_t_guards(eng):
    lib = eng.lib()
    a = np.zeros((4, 4))
    x = np.zeros((4, 2))
    b = np.zeros((4, 2))
    r = np.zeros((4, 2))
    ok = (4, 4, 2, 4, _p(a), _p(x), _p(b), _p(r))
    assert lib.conflux_lu_debug_residual_dd_t(*ok) == 0
    for i, bad in ((0, 0), (1, 0), (2, 0), (0, -1), (3, 3), (4, None),
                   (5, None), (6, None), (7, None)):
        args = list(ok)
        args[i] = bad
        assert lib.conflux_lu_debug_residual_dd_t(*args) == EARG, i


# ---------------- exact recovery, transposed --------------------------------

def _int_system(N, dens, seed, nrhs):
    """A = P L U with small integer factors: exactly representable, cond
    ~1e7, integer solution."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-1, 2, (N, N)) * (rng.random((N, N)) < dens),
                -1) + np.eye(N, dtype=np.int64)
    Uf = np.triu(rng.integers(-1, 2, (N, N)) * (rng.random((N, N)) < dens),
                 1) + np.diag(rng.choice([-1, 1], N))
    A = (L.astype(np.int64) @ Uf.astype(np.int64))[rng.permutation(N)]
    Xt = np.random.default_rng(50 + seed).integers(-1000, 1001, (N, nrhs))
    B = A @ Xt
    assert np.abs(A).max() < 2 ** 30 and np.abs(B).max() < 2 ** 53
    return A.astype(np.float64), Xt.astype(np.float64), B.astype(np.float64)


@pytest.mark.parametrize("Px,Py,Pz", GRIDS)
@pytest.mark.parametrize("N,dens", [(128, 0.15), (256, 0.08)])
def test_refine_trans_recovers_integer_solution_exactly(eng, N, dens, Px, Py,
                                                        Pz):
    """A^T X = B with B = A^T Xt exact in integers, cond ~1e7: the plain
    transposed solve loses 6-7 digits (asserted: the case is hard), the
    refined one returns Xt bit for bit in at most 4 passes."""
    with eng.Engine(N, 32, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        A = _int_system(N, dens, 0, 1)[0]
        e.set_matrix_global(A)
        e.factor()
        for nrhs in (1, 3):
            A, Xt, _ = _int_system(N, dens, 0, nrhs)
            Bi = A.T.astype(np.int64) @ Xt.astype(np.int64)
            assert np.abs(Bi).max() < 2 ** 53
            B = Bi.astype(np.float64)
            X0 = e.solve_transposed_refined(B, max_iter=0)
            assert hp.bits_equal(X0, e.solve_transposed(B))
            f0 = np.abs(X0 - Xt).max() / np.abs(Xt).max()
            X, info = e.solve_transposed_refined(B, max_iter=10,
                                                 return_info=True)
            print(f"int^T N={N} {Px}x{Py}x{Pz} nrhs={nrhs}: plain "
                  f"ferr={f0:.3g} refined maxdiff={np.abs(X - Xt).max():.3g} "
                  f"{info}")
            assert f0 >= 1e-12
            assert np.array_equal(X, Xt)
            assert (info["berr"] == 0.0).all()
            assert info["iters"] <= 4


# ---------------- the no-pivot path is rescued, transposed ------------------

def _berr_host(A, X, B):
    """The engine's berr formula with an np.longdouble residual (0 where
    the denominator is 0, as the engine defines it)."""
    Al, Xl, Bl = (np.asarray(t, dtype=np.longdouble) for t in (A, X, B))
    R = np.abs(Bl - Al @ Xl).max(axis=0)
    den = np.abs(Al).sum(axis=1).max() * np.abs(Xl).max(axis=0) + \
        np.abs(Bl).max(axis=0)
    safe = np.where(den == 0, 1, den)
    return np.asarray(np.where(den == 0, 0, R / safe), dtype=np.float64)


def _berr_close(b, bh, n):
    return (np.abs(b - bh) <= 1e-3 * b + (n + 2) * 2.0 ** -64).all()


@pytest.mark.parametrize("Px,Py,Pz", GRIDS)
def test_refine_trans_rescues_nopivot(eng, Px, Py, Pz):
    """test_refine_rescues_nopivot's matrix and factorization, solved for
    A^T: refinement brings the backward error below numpy's for
    solve(A.T, B), the plain transposed solve is at least 100x worse, and
    the reported berr (||A^T||inf = ||A||1) agrees with the host's
    longdouble evaluation."""
    N = 256
    A = np.random.default_rng(0).standard_normal((N, N))
    with eng.Engine(N, 32, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(A)
        e.factor()
        for nrhs in (1, 17):
            B = np.random.default_rng(nrhs).standard_normal((N, nrhs))
            X0, i0 = e.solve_transposed_refined(B, max_iter=0,
                                                return_info=True)
            X1, i1 = e.solve_transposed_refined(B, max_iter=10,
                                                return_info=True)
            b0, b1 = i0["berr"], i1["berr"]
            bnp = _berr_host(A.T, np.linalg.solve(A.T, B), B)
            print(f"nopiv^T {Px}x{Py}x{Pz} nrhs={nrhs}: b0={b0.min():.3g}.."
                  f"{b0.max():.3g} b1={b1.min():.3g}..{b1.max():.3g} "
                  f"numpy={bnp.min():.3g}..{bnp.max():.3g} "
                  f"iters={i1['iters']} ferr={i1['ferr'].max():.3g}")
            assert (b1 <= bnp).all()
            assert (b0 >= 100 * b1).all()
            for X, b in ((X0, b0), (X1, b1)):
                bh = _berr_host(A.T, X, B)
                print(f"   engine berr vs host: max |diff|="
                      f"{np.abs(b - bh).max():.3g}")
                assert _berr_close(b, bh, N)


# ---------------- device B equals host B at n == N_padded -------------------

def _spd(N):
    G = gen_matrix(N)
    return 0.5 * (G + G.T) + 2.0 * N * np.eye(N)


def _get_inputs(eng, e):
    out = []
    for g in range(e.Px * e.Py * e.Pz if e.sim else 1):
        loc = np.full((e.Ml, e.Nl), np.nan)
        assert eng.lib().conflux_lu_debug_get_input(e._h, g, _p(loc)) == 0
        out.append(loc)
    return out


@pytest.mark.parametrize("kind", ["lu", "lu_trans", "chol"])
@pytest.mark.parametrize("mode,N,v,P", [("sim", 256, 32, 2),
                                        ("real", 512, 64, 1)])
def test_device_equals_host_full_order(eng, torch, mode, N, v, P, kind):
    """After set_matrix_device with n == N_padded the device entry returns
    X, berr, ferr and iters bitwise equal to the host entry's; max_iter = 0
    on device is the unrefined device solve; factors and snapshot are only
    read."""
    chol = kind == "chol"
    A = _spd(N) if chol else gen_matrix(N)
    B = np.random.default_rng(N + len(kind)).standard_normal((N, 5))
    kw = dict(rank=-1) if mode == "sim" else dict(rank=0, world=1)
    with eng.Engine(N, v, P, P, 1, **kw) as e:
        e.store_factors(True)
        tA = _dev(torch, A)
        e.set_matrix_device(tA.data_ptr(), N, N, 0)
        assert e.n == e.Npad == N
        e.factor_cholesky() if chol else e.factor()
        getF = e.get_F_global if mode == "sim" else e.get_F_local
        F0, S0 = getF().copy(), _get_inputs(eng, e)
        host = {"lu": e.solve_refined, "lu_trans": e.solve_transposed_refined,
                "chol": e.solve_cholesky_refined}[kind]

        def device(t, max_iter):
            if chol:
                return e.solve_cholesky_refined_device(t.data_ptr(), 5, 5,
                                                       max_iter=max_iter)
            return e.solve_refined_device(t.data_ptr(), 5, 5,
                                          trans=kind == "lu_trans",
                                          max_iter=max_iter)

        def plain(t):
            if chol:
                return e.solve_cholesky_device(t.data_ptr(), 5, 5)
            return e.solve_device(t.data_ptr(), 5, 5,
                                  trans=kind == "lu_trans")

        for max_iter in (10, 1, 0):
            Xh, ih = host(B, max_iter=max_iter, return_info=True)
            t = _dev(torch, B)
            idv = device(t, max_iter)
            Xd = _host(torch, t)
            assert hp.bits_equal(Xd, Xh), (kind, max_iter)
            assert hp.bits_equal(idv["berr"], ih["berr"])
            assert hp.bits_equal(idv["ferr"], ih["ferr"])
            assert idv["iters"] == ih["iters"]
            assert idv["berr"].shape == (5,) and idv["ms"] > 0
        t = _dev(torch, B)
        plain(t)
        assert hp.bits_equal(Xd, _host(torch, t)), "max_iter=0 != plain"
        assert np.array_equal(F0, getF()), "refinement wrote Fres"
        for s0, s1 in zip(S0, _get_inputs(eng, e)):
            assert np.array_equal(s0, s1), "refinement wrote the snapshot"


# ---------------- logical order n < N_padded, through conflux_amd.dense -----

def _tensor(torch, A, order):
    """A on the device, row-major (order 0) or column-major (order 1)."""
    if order == 0:
        return _dev(torch, A)
    return _dev(torch, np.ascontiguousarray(A.T)).T


@pytest.mark.parametrize("nrhs", [1, 17])
@pytest.mark.parametrize("n,order,scale", [(50, 0, 1e-3), (250, 0, 1.0),
                                           (250, 1, 1.0)])
def test_dense_refine_logical_order(eng, torch, n, order, scale, nrhs):
    """n = 50 pads to 64 and n = 250 to 256 with v = 32.  Refined berr is at
    most numpy's on the n x n system and agrees with the host's longdouble
    evaluation on the n x n matrices — the norm is the leading block's, not
    blockdiag(A, I)'s: with scale = 1e-3, ||A|| < 1 and the padding's 1
    would win.  B is untouched, refine=False is today's solve bit for bit,
    and a zero column comes back zero with berr 0."""
    from conflux_amd import dense
    rng = np.random.default_rng(7 * n + nrhs + order)
    A = scale * rng.standard_normal((n, n))
    S = scale * _spd(n)
    if scale != 1.0:
        assert np.abs(A).sum(axis=1).max() < 1 and \
            np.abs(A).sum(axis=0).max() < 1
    B = rng.standard_normal((n, nrhs))
    if nrhs > 1:
        B[:, 3] = 0.0
    tB = _dev(torch, B)
    cases = [
        ("nopiv", lambda: dense.lu_factor(_tensor(torch, A, order), v=32,
                                          pivot=False), "solve", A),
        ("trans", lambda: dense.lu_factor(_tensor(torch, A, order), v=32),
         "solve_transposed", A.T),
        ("chol", lambda: dense.cholesky_factor(_tensor(torch, S, order),
                                               v=32), "solve", S),
    ]
    for tag, factor, method, Aeff in cases:
        with factor() as f:
            assert f._e.Npad == (64 if n == 50 else 256) and f._e.n == n
            solve = getattr(f, method)
            X, info = solve(tB, refine=True, return_info=True)
            assert hp.bits_equal(_host(torch, tB), B), "B was modified"
            Xn = _host(torch, X)
            b = info["berr"].numpy()
            assert info["berr"].dtype == torch.float64 and \
                info["ferr"].dtype == torch.float64
            assert not info["berr"].is_cuda and not info["ferr"].is_cuda
            assert tuple(info["berr"].shape) == (nrhs,) and \
                tuple(info["ferr"].shape) == (nrhs,)
            assert isinstance(info["iters"], int)
            bnp = _berr_host(Aeff, np.linalg.solve(Aeff, B), B)
            bh = _berr_host(Aeff, Xn, B)
            print(f"dense {tag} n={n} order={order} nrhs={nrhs}: "
                  f"berr={b.max():.3g} numpy={bnp.min():.3g}.."
                  f"{bnp.max():.3g} host={bh.max():.3g} "
                  f"iters={info['iters']}")
            assert (b <= bnp).all()
            assert _berr_close(b, bh, n)
            if nrhs > 1:
                assert not Xn[:, 3].any() and b[3] == 0.0
            # refine off: today's path, and its figures on request
            Xp = solve(tB)
            t = tB.clone()
            torch.cuda.synchronize()
            if tag == "chol":
                f._e.solve_cholesky_device(t.data_ptr(), nrhs, nrhs)
            else:
                f._e.solve_device(t.data_ptr(), nrhs, nrhs,
                                  trans=tag == "trans")
            assert hp.bits_equal(_host(torch, Xp), _host(torch, t))
            for off in (False, 0):
                X0, i0 = solve(tB, refine=off, return_info=True)
                assert hp.bits_equal(_host(torch, X0), _host(torch, Xp))
                assert i0["iters"] == 0
                assert _berr_close(i0["berr"].numpy(),
                                   _berr_host(Aeff, _host(torch, X0), B), n)
            assert hp.bits_equal(_host(torch, solve(tB, refine=10)), Xn)
            with pytest.raises(ValueError):
                solve(tB, refine=-1)
            # 1-D round trip
            b1 = tB[:, 0].contiguous()
            x1, i1 = solve(b1, refine=True, return_info=True)
            assert tuple(x1.shape) == (n,) and \
                tuple(i1["berr"].shape) == (1,)
            assert hp.bits_equal(_host(torch, x1), Xn[:, 0])


# ---------------- slack and guards ------------------------------------------

@pytest.mark.parametrize("kind", ["lu", "lu_trans", "chol"])
def test_device_slack_untouched(eng, torch, kind):
    """ldb = nrhs + 3: the slack of every row holds its canaries afterwards,
    at a logical order below the padded one."""
    n, nrhs = 50, 4
    chol = kind == "chol"
    A = _spd(n) if chol else gen_matrix(n)
    B = np.random.default_rng(3).standard_normal((n, nrhs))
    with eng.Engine(64, 32, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        tA = _dev(torch, A)
        e.set_matrix_device(tA.data_ptr(), n, n, 0)
        assert e.n == n and e.Npad == 64
        e.factor_cholesky() if chol else e.factor()
        t = _dev(torch, hp.framed(B, n, nrhs + 3))
        if chol:
            info = e.solve_cholesky_refined_device(t.data_ptr(), nrhs + 3,
                                                   nrhs)
        else:
            info = e.solve_refined_device(t.data_ptr(), nrhs + 3, nrhs,
                                          trans=kind == "lu_trans")
        out = _host(torch, t)
        assert hp.frame_intact(out, n, nrhs)
        Aeff = A.T if kind == "lu_trans" else A
        assert _berr_close(info["berr"],
                           _berr_host(Aeff, out[:, :nrhs], B), n)


def test_refined_device_guards(eng, torch):
    lib = eng.lib()
    N, v = 64, 8
    B = np.ones((N, 2))
    t = _dev(torch, B)
    d = t.data_ptr()
    ms = ctypes.c_double()
    it = ctypes.c_int()
    be = np.zeros(2)
    fe = np.zeros(2)
    lud = lib.conflux_lu_solve_refined_device
    chd = lib.conflux_chol_solve_refined_device
    lut = lib.conflux_lu_solve_refined_trans
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.set_matrix_global(gen_matrix(N))
        # before any factorization
        assert lud(e._h, d, 2, 2, 0, 3, _p(be), _p(fe), ctypes.byref(it),
                   ctypes.byref(ms)) == EARG
        assert chd(e._h, d, 2, 2, 3, None, None, None, None) == EARG
        assert lut(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        # last factorization ran with store_factors off
        e.store_factors(False)
        e.factor()
        assert lud(e._h, d, 2, 2, 0, 3, None, None, None, None) == EARG
        assert lut(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        e.store_factors(True)
        e.factor()
        assert lud(e._h, d, 1, 2, 0, 3, None, None, None, None) == EARG  # ldb
        assert lud(e._h, d, 2, 2, 2, 3, None, None, None, None) == EARG
        assert lud(e._h, d, 2, 2, -1, 3, None, None, None, None) == EARG
        assert lud(e._h, d, 2, 2, 0, -1, None, None, None, None) == EARG
        assert lud(e._h, d, 2, 0, 0, 3, None, None, None, None) == EARG
        assert lud(e._h, None, 2, 2, 0, 3, None, None, None, None) == EARG
        assert lut(e._h, _p(B), 2, -1, None, None, None, None) == EARG
        assert lut(e._h, None, 2, 3, None, None, None, None) == EARG
        assert lut(e._h, _p(B), 0, 3, None, None, None, None) == EARG
        # kind mismatch
        assert chd(e._h, d, 2, 2, 3, None, None, None, None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.solve_cholesky_refined_device(d, 2, 2)
        with pytest.raises(eng.ConfluxLuError):
            e.solve_refined_device(d, 2, 2, max_iter=-1)
        # the guards left B alone and the engine usable; every out pointer
        # may be NULL
        assert np.array_equal(B, np.ones((N, 2)))
        assert np.array_equal(_host(torch, t), np.ones((N, 2)))
        for trans in (0, 1):
            t2 = _dev(torch, B)
            assert lud(e._h, t2.data_ptr(), 2, 2, trans, 3, None, None, None,
                       None) == 0
            t2 = _dev(torch, B)
            assert lud(e._h, t2.data_ptr(), 2, 2, trans, 0, _p(be), None,
                       ctypes.byref(it), None) == 0
            assert it.value == 0 and np.isfinite(be).all() and \
                (be >= 0).all()
        assert lut(e._h, _p(B.copy()), 2, 3, None, None, None, None) == 0
        # a store_factors-off run invalidates the earlier factors
        e.store_factors(False)
        e.factor()
        assert lud(e._h, d, 2, 2, 0, 3, None, None, None, None) == EARG
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(_spd(N))
        e.factor_cholesky()
        assert lud(e._h, d, 2, 2, 0, 3, None, None, None, None) == EARG
        assert lut(e._h, _p(B), 2, 3, None, None, None, None) == EARG
        with pytest.raises(eng.ConfluxLuError):
            e.solve_transposed_refined(B)
        assert chd(e._h, None, 2, 2, 3, None, None, None, None) == EARG
        assert chd(e._h, d, 1, 2, 3, None, None, None, None) == EARG
        assert chd(e._h, d, 2, 0, 3, None, None, None, None) == EARG
        assert chd(e._h, d, 2, 2, -1, None, None, None, None) == EARG
        t2 = _dev(torch, B)
        assert chd(e._h, t2.data_ptr(), 2, 2, 3, None, None, None, None) == 0
