"""GPU tests of the device-resident dense interface
(conflux_lu_set_matrix_device / get_factors_device / solve_device /
chol_solve_device / slogdet / chol_logdet / logical_order, the logical-order
rcond, and conflux_amd.dense).

The caller's n x n device matrix enters as blockdiag(A, I) of the padded
order; every check is against numpy on the n x n A.  Inputs live in torch
device tensors; multi-rank grids use the single-process simulation mode.
The input snapshot is read back through conflux_lu_debug_get_input, a test
hook added with this interface (no host path returned the snapshot before).
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
# torch before the engine's library is loaded anywhere in this process (test
# modules are imported at collection, before any test runs): a torch wheel
# that bundles its own HIP runtime must load it first, so that the engine
# binds to that same copy — two HIP runtimes in one process cannot both open
# the GPU (conflux_amd/dense.py says the same to its users).
import torch as _torch  # noqa: F401

pytestmark = pytest.mark.gpu

from oracle import gen_matrix  # noqa: E402

EARG = -1
EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "shimccl.so")

# (n, v, Px, Pz): exact fit, one / 31 / 63 columns over a tile, two ranks per
# side, a whole tile of padding on a 2x2x2 grid, v = 8 (tile smaller than the
# transpose's 32), and v = 128 with n far from a tile edge
SHAPES = [(64, 32, 1, 1), (65, 32, 1, 1), (95, 32, 1, 1), (33, 32, 1, 1),
          (97, 32, 2, 1), (130, 32, 2, 2), (40, 8, 1, 1), (300, 128, 1, 1)]
PADDED = [s for s in SHAPES if s[0] != 64]
SOLVE_SHAPES = [(65, 32, 1, 1), (97, 32, 2, 1), (130, 32, 2, 2),
                (300, 128, 1, 1), (1000, 256, 1, 1)]
NRHS = [1, 3, 17, 130]


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


@pytest.fixture(scope="module")
def torch():
    return _torch


def _mat(n):
    return gen_matrix(n)


def _dd(n):  # diagonally dominant, for the no-pivot path
    return gen_matrix(n) + 6.0 * n * np.eye(n)


def _spd(n):
    G = gen_matrix(n)
    return 0.5 * (G + G.T) + 2.0 * n * np.eye(n)


def _upload(torch, A, order=0, extra=0):
    """A as a device buffer with leading dimension n + extra in the given
    order; the slack holds NaN.  Returns (tensor, lda)."""
    n = A.shape[0]
    W = np.full((n, n + extra), np.nan)
    W[:, :n] = A if order == 0 else A.T
    return torch.from_numpy(W).cuda(), n + extra


def _engine(eng, shape):
    n, v, Px, Pz = shape
    e = eng.Engine(n, v, Px, Px, Pz, rank=-1)
    e.store_factors(True)
    return e


def _set(e, t, lda, n, order=0):
    e.set_matrix_device(t.data_ptr(), lda, n, order)


def _factored(eng, torch, shape, A, chol=False, pivot=True):
    e = _engine(eng, shape)
    t, lda = _upload(torch, A)
    _set(e, t, lda, A.shape[0])
    e.set_pivoting(1 if pivot else 0)
    e.factor_cholesky() if chol else e.factor()
    return e


def _blockdiag(A, N):
    G = np.eye(N)
    G[:A.shape[0], :A.shape[0]] = A
    return G


def _local(G, v, Px, pi, pj):
    Nt = G.shape[0] // v
    rows = np.concatenate([np.arange(t * v, (t + 1) * v)
                           for t in range(pi, Nt, Px)])
    cols = np.concatenate([np.arange(t * v, (t + 1) * v)
                           for t in range(pj, Nt, Px)])
    return G[np.ix_(rows, cols)]


def _get_input(eng, e, g):
    loc = np.full((e.Ml, e.Nl), np.nan)
    assert eng.lib().conflux_lu_debug_get_input(
        e._h, g, loc.ctypes.data_as(ctypes.c_void_p)) == 0
    return loc


def _eta(A, X, B):
    return np.linalg.norm(B - A @ X) / (
        np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(B))


def _check_eta(A, X, B, tag):
    eta = _eta(A, X, B)
    eta_np = _eta(A, np.linalg.solve(A, B), B)
    print(f"{tag}: eta={eta:.3g} eta_numpy={eta_np:.3g} "
          f"ratio={eta / eta_np:.2f}")
    assert eta <= 10 * eta_np, f"{tag}: eta={eta} vs numpy {eta_np}"


# ---------------- 1. import --------------------------------------------------

@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_import_exact(eng, torch, shape, order, extra):
    """The snapshot every rank keeps equals its tile-cyclic share of
    blockdiag(A, I) bitwise; pk > 0 layers hold zeros.  lda = n + 3 is odd
    for even n (the scalar row-major path) and leaves NaN slack that must not
    leak."""
    n, v, Px, Pz = shape
    A = _mat(n)
    with _engine(eng, shape) as e:
        t, lda = _upload(torch, A, order, extra)
        _set(e, t, lda, n, order)
        assert e.n == n
        e.factor()
        G = _blockdiag(A, e.Npad)
        for pi in range(Px):
            for pj in range(Px):
                for pk in range(Pz):
                    got = _get_input(eng, e, (pi * Px + pj) * Pz + pk)
                    want = _local(G, v, Px, pi, pj) if pk == 0 else \
                        np.zeros((e.Ml, e.Nl))
                    assert np.array_equal(got, want), (shape, pi, pj, pk)


@pytest.mark.parametrize("shape", [(64, 32, 1, 1), (128, 32, 2, 2)])
@pytest.mark.parametrize("order", [0, 1])
def test_import_matches_host_upload(eng, torch, shape, order):
    """No padding: the device import and set_matrix_global of the same A
    factor to the same bits."""
    n = shape[0]
    A = _mat(n)
    with _engine(eng, shape) as e:
        t, lda = _upload(torch, A, order)
        _set(e, t, lda, n, order)
        e.factor()
        F1, p1 = e.get_F_global(), e.get_perm()
        e.set_matrix_global(A)
        assert e.n == e.Npad
        e.factor()
        assert np.array_equal(F1, e.get_F_global())
        assert np.array_equal(p1, e.get_perm())


# ---------------- 2. padding is inert ----------------------------------------

@pytest.mark.parametrize("shape", PADDED)
def test_padding_inert_and_export(eng, torch, shape):
    import scipy.linalg as la
    n = shape[0]
    A = _mat(n)
    with _factored(eng, torch, shape, A) as e:
        N = e.Npad
        F, perm = e.get_F_global(), e.get_perm()
        assert np.array_equal(perm[n:], np.arange(n, N))
        assert sorted(perm[:n]) == list(range(n))
        assert np.array_equal(F[n:, n:], np.eye(N - n))
        assert not F[:n, n:].any() and not F[n:, :n].any()
        for ldf in (n, n + 5):
            dF = torch.full((n, ldf), float("nan"), dtype=torch.float64,
                            device="cuda")
            dp = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            e.get_factors_device(dF.data_ptr(), ldf, dp.data_ptr())
            hF = dF.cpu().numpy()
            assert np.array_equal(hF[:, :n], F[:n, :n]), (shape, ldf)
            assert np.isnan(hF[:, n:]).all(), "export wrote into the slack"
            assert np.array_equal(dp.cpu().numpy(), perm[:n])
            e.get_factors_device(dF.data_ptr(), ldf, None)
            e.get_factors_device(None, 0, dp.data_ptr())
        L = np.tril(hF[:, :n], -1) + np.eye(n)
        U = np.triu(hF[:, :n])
        res = np.linalg.norm(A[perm[:n]] - L @ U) / np.linalg.norm(A)
        lu, piv = la.lu_factor(A)
        Lr, Ur = np.tril(lu, -1) + np.eye(n), np.triu(lu)
        PA = A.copy()
        for i, p in enumerate(piv):
            PA[[i, p]] = PA[[p, i]]
        res_ref = np.linalg.norm(PA - Lr @ Ur) / np.linalg.norm(A)
        print(f"{shape}: ||PA-LU||/||A|| = {res:.3g}, scipy {res_ref:.3g}")
        assert res <= 10 * res_ref


# ---------------- 3. solves --------------------------------------------------

def _solve_dev(torch, e, B, extra, call):
    """Run an in-place device solve on B inside a buffer with ldb = nrhs +
    extra; returns X and checks that the slack is untouched."""
    n, nrhs = B.shape
    W = np.full((n, nrhs + extra), -7.25)
    W[:, :nrhs] = B
    t = torch.from_numpy(W).cuda()
    torch.cuda.synchronize()
    ms = call(t.data_ptr(), nrhs + extra, nrhs)
    assert ms > 0
    out = t.cpu().numpy()
    assert (out[:, nrhs:] == -7.25).all(), "solve wrote into the ldb slack"
    return np.ascontiguousarray(out[:, :nrhs])


@pytest.mark.parametrize("shape", SOLVE_SHAPES)
def test_solve_device(eng, torch, shape):
    n = shape[0]
    A = _mat(n)
    rng = np.random.default_rng(n)
    with _factored(eng, torch, shape, A) as e:
        F0 = e.get_F_global().copy()
        for nrhs in NRHS:
            B = rng.standard_normal((n, nrhs))
            for extra in (0, 2):
                X = _solve_dev(torch, e, B, extra, e.solve_device)
                _check_eta(A, X, B, f"dev {shape} nrhs={nrhs} +{extra}")
                Xt = _solve_dev(
                    torch, e, B, extra,
                    lambda p, ld, k: e.solve_device(p, ld, k, trans=True))
                _check_eta(A.T, Xt, B, f"devT {shape} nrhs={nrhs} +{extra}")
            X2 = _solve_dev(torch, e, B, 0, e.solve_device)
            assert np.array_equal(X, X2), "two calls differ"
        assert np.array_equal(F0, e.get_F_global()), "solve wrote into Fres"


@pytest.mark.parametrize("shape", [(65, 32, 1, 1), (130, 32, 2, 2),
                                   (300, 128, 1, 1)])
def test_solve_device_nopivot_and_cholesky(eng, torch, shape):
    n = shape[0]
    rng = np.random.default_rng(n + 1)
    B = rng.standard_normal((n, 17))
    A = _dd(n)
    with _factored(eng, torch, shape, A, pivot=False) as e:
        assert np.array_equal(e.get_perm(), np.arange(e.Npad))
        for extra in (0, 2):
            X = _solve_dev(torch, e, B, extra, e.solve_device)
            _check_eta(A, X, B, f"nopiv {shape}")
            Xt = _solve_dev(
                torch, e, B, extra,
                lambda p, ld, k: e.solve_device(p, ld, k, trans=True))
            _check_eta(A.T, Xt, B, f"nopivT {shape}")
    S = _spd(n)
    with _factored(eng, torch, shape, S, chol=True) as e:
        for nrhs in (1, 17, 130):
            B = rng.standard_normal((n, nrhs))
            for extra in (0, 2):
                X = _solve_dev(torch, e, B, extra, e.solve_cholesky_device)
                _check_eta(S, X, B, f"chol {shape} nrhs={nrhs}")
        X2 = _solve_dev(torch, e, B, 0, e.solve_cholesky_device)
        assert np.array_equal(
            X2, _solve_dev(torch, e, B, 0, e.solve_cholesky_device))


@pytest.mark.parametrize("shape", [(64, 32, 1, 1), (128, 32, 2, 2)])
def test_solve_device_equals_host_bitwise(eng, torch, shape):
    n = shape[0]
    rng = np.random.default_rng(5)
    with _factored(eng, torch, shape, _mat(n)) as e:
        for nrhs in (1, 17):
            B = rng.standard_normal((n, nrhs))
            assert np.array_equal(
                _solve_dev(torch, e, B, 2, e.solve_device), e.solve(B))
            assert np.array_equal(
                _solve_dev(torch, e, B, 2,
                           lambda p, ld, k: e.solve_device(p, ld, k, True)),
                e.solve_transposed(B))
    with _factored(eng, torch, shape, _spd(n), chol=True) as e:
        B = rng.standard_normal((n, 3))
        assert np.array_equal(
            _solve_dev(torch, e, B, 2, e.solve_cholesky_device),
            e.solve_cholesky(B))


# ---------------- 4. determinants --------------------------------------------

def _logdet_tol(A, ref):
    """What rounding alone does to log|det A| for this input: the spread
    between numpy's value for A and for A with its rows reversed (the same
    matrix under another pivot order), times 10, floored at n eps |ref|."""
    other = np.linalg.slogdet(A[::-1])[1]
    return max(10 * abs(ref - other), A.shape[0] * EPS * abs(ref))


@pytest.mark.parametrize("shape", [(64, 32, 1, 1), (65, 32, 1, 1),
                                   (97, 32, 2, 1), (130, 32, 2, 2),
                                   (300, 128, 1, 1)])
def test_slogdet(eng, torch, shape):
    n = shape[0]
    A = np.random.default_rng(40 + n).standard_normal((n, n))
    sg_np, ld_np = np.linalg.slogdet(A)
    with _factored(eng, torch, shape, A) as e:
        sg, ld = e.slogdet()
        d = np.diag(e.get_F_global())[:n]
        logs = np.log(np.abs(d))
        exact = math.fsum(logs)
        tol_sum = 4 * n * EPS * np.abs(logs).max()
        tol_np = _logdet_tol(A, ld_np)
        print(f"{shape}: sign={sg} logabsdet={ld!r} fsum={exact!r} "
              f"numpy={ld_np!r} |d fsum|={abs(ld - exact):.3g} (tol "
              f"{tol_sum:.3g}) |d numpy|={abs(ld - ld_np):.3g} (tol "
              f"{tol_np:.3g})")
        assert sg == sg_np
        assert abs(ld - exact) <= tol_sum
        assert abs(ld - ld_np) <= tol_np
        assert e.slogdet() == (sg, ld), "two calls differ"
        # a row swap flips the sign
        A2 = A.copy()
        A2[[0, 1]] = A2[[1, 0]]
        t, lda = _upload(torch, A2)
        _set(e, t, lda, n)
        e.factor()
        sg2, ld2 = e.slogdet()
        assert sg2 == -sg
        assert abs(ld2 - ld_np) <= tol_np
        # a zero on U's diagonal: singular, not an error
        k = n // 2
        dk = e.get_F_global()[k, k]
        assert eng.lib().conflux_lu_debug_poke_factor(e._h, k, k, -dk) == 0
        assert e.slogdet() == (0.0, -math.inf)


@pytest.mark.parametrize("shape", [(65, 32, 1, 1), (130, 32, 2, 2)])
def test_logdet_cholesky(eng, torch, shape):
    n = shape[0]
    S = _spd(n)
    sg_np, ld_np = np.linalg.slogdet(S)
    assert sg_np == 1.0
    with _factored(eng, torch, shape, S, chol=True) as e:
        ld = e.logdet_cholesky()
        d = np.diag(e.get_F_global())[:n]
        logs = np.log(np.abs(d))
        assert abs(ld - 2 * math.fsum(logs)) <= \
            2 * 4 * n * EPS * np.abs(logs).max()
        assert abs(ld - ld_np) <= _logdet_tol(S, ld_np)
        assert e.logdet_cholesky() == ld
        sg = ctypes.c_double()
        assert eng.lib().conflux_lu_slogdet(
            e._h, ctypes.byref(sg), ctypes.byref(sg)) == EARG


# ---------------- 5. rcond of the n x n matrix -------------------------------

def _check_rcond(A, which, rc, info, tag):
    n = A.shape[0]
    p = 1 if which == "1" else np.inf
    anorm = np.linalg.norm(A, p)
    true = 1.0 / (anorm * np.linalg.norm(np.linalg.inv(A), p))
    ratio = rc / true
    print(f"{tag} norm={which}: rcond={rc:.6g} true={true:.6g} "
          f"ratio={ratio:.6f} anorm={info['anorm']!r} numpy={anorm!r}")
    assert 1 - 1e-3 <= ratio <= 3, (tag, which, ratio)
    assert abs(info["anorm"] - anorm) <= n * EPS * anorm, (tag, which)
    assert 1 <= info["nsolves"] <= 12


@pytest.mark.parametrize("shape", [(65, 32, 1, 1), (97, 32, 2, 1)])
def test_rcond_logical_order(eng, torch, shape):
    """A is scaled so every one of its column and row sums is below 1: a
    padding column (sum exactly 1) would win an unrestricted norm."""
    n = shape[0]
    A = 1e-3 * _mat(n)
    assert np.linalg.norm(A, 1) < 1 and np.linalg.norm(A, np.inf) < 1
    with _factored(eng, torch, shape, A) as e:
        for which in ("1", "I"):
            rc, info = e.rcond(which, return_info=True)
            _check_rcond(A, which, rc, info, f"rcond {shape}")
            assert e.rcond(which) == rc
    S = 1e-3 * _spd(n) / n
    assert np.linalg.norm(S, 1) < 1
    with _factored(eng, torch, shape, S, chol=True) as e:
        rc, info = e.rcond_cholesky(return_info=True)
        _check_rcond(S, "1", rc, info, f"rcond chol {shape}")


def test_rcond_full_order_unchanged(eng, torch):
    shape = (64, 32, 1, 1)
    A = _mat(64)
    with _factored(eng, torch, shape, A) as e:
        got = [e.rcond(w, return_info=True) for w in ("1", "I")]
        e.set_matrix_global(A)
        e.factor()
        for w, (rc, info) in zip(("1", "I"), got):
            rc2, info2 = e.rcond(w, return_info=True)
            assert rc == rc2 and info["anorm"] == info2["anorm"]
            assert info["nsolves"] == info2["nsolves"]


# ---------------- 6. guards --------------------------------------------------

def test_dense_guards(eng, torch):
    lib = eng.lib()
    n = 65
    A = _mat(n)
    t, lda = _upload(torch, A)
    B = torch.ones((n, 4), dtype=torch.float64, device="cuda")
    dF = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pA, pB, pF = t.data_ptr(), B.data_ptr(), dF.data_ptr()
    x = ctypes.c_double()
    y = ctypes.c_double()
    rx, ry = ctypes.byref(x), ctypes.byref(y)
    with _engine(eng, (n, 32, 1, 1)) as e:
        h, N = e._h, e.Npad
        assert e.n == N
        # nothing factored yet
        assert lib.conflux_lu_solve_device(h, pB, 4, 4, 0, None) == EARG
        assert lib.conflux_chol_solve_device(h, pB, 4, 4, None) == EARG
        assert lib.conflux_lu_slogdet(h, rx, ry) == EARG
        assert lib.conflux_chol_logdet(h, rx) == EARG
        assert lib.conflux_lu_get_factors_device(h, pF, n, None) == EARG
        # set_matrix_device arguments
        sm = lib.conflux_lu_set_matrix_device
        assert sm(h, None, lda, n, 0) == EARG
        assert sm(h, pA, n - 1, n, 0) == EARG
        assert sm(h, pA, lda, n, 2) == EARG
        assert sm(h, pA, lda, n, -1) == EARG
        assert sm(h, pA, lda, 0, 0) == EARG
        assert sm(h, pA, N + 1, N + 1, 0) == EARG
        assert e.n == N, "a refused call changed the logical order"
        assert lib.conflux_lu_logical_order(h, None) == EARG
        assert sm(h, pA, lda, n, 0) == 0
        assert e.n == n
        e.init_matrix(3)
        assert e.n == N, "init_matrix must reset the logical order"
        assert sm(h, pA, lda, n, 0) == 0
        e.factor()
        # solve arguments
        sd = lib.conflux_lu_solve_device
        assert sd(h, None, 4, 4, 0, None) == EARG
        assert sd(h, pB, 3, 4, 0, None) == EARG
        assert sd(h, pB, 4, 0, 0, None) == EARG
        assert sd(h, pB, 4, 4, 2, None) == EARG
        assert sd(h, pB, 4, 4, -1, None) == EARG
        assert lib.conflux_chol_solve_device(h, pB, 4, 4, None) == EARG
        assert lib.conflux_chol_logdet(h, rx) == EARG
        assert lib.conflux_lu_slogdet(h, None, ry) == EARG
        assert lib.conflux_lu_slogdet(h, rx, None) == EARG
        assert lib.conflux_lu_get_factors_device(h, pF, n - 1, None) == EARG
        assert (B.cpu().numpy() == 1.0).all(), "a refused solve wrote B"
        assert sd(h, pB, 4, 4, 0, None) == 0
        assert lib.conflux_lu_slogdet(h, rx, ry) == 0
        # a Cholesky factorization: the LU calls refuse
        tS, ldS = _upload(torch, _spd(n))
        _set(e, tS, ldS, n)
        e.factor_cholesky()
        assert sd(h, pB, 4, 4, 0, None) == EARG
        assert lib.conflux_lu_slogdet(h, rx, ry) == EARG
        assert lib.conflux_chol_solve_device(h, None, 4, 4, None) == EARG
        assert lib.conflux_chol_solve_device(h, pB, 3, 4, None) == EARG
        assert lib.conflux_chol_logdet(h, None) == EARG
        assert lib.conflux_chol_logdet(h, rx) == 0
        # store_factors off: nothing to solve with
        e.store_factors(False)
        e.factor()
        assert sd(h, pB, 4, 4, 0, None) == EARG
        assert lib.conflux_lu_slogdet(h, rx, ry) == EARG
        assert lib.conflux_lu_get_factors_device(h, pF, n, None) == EARG


def test_dense_refuse_world_2(tmp_path):
    """Two real ranks (1x1x2 grid, shimccl transport): every entry point of
    the dense interface returns EARG on every rank, before any
    communication, and leaves the buffers alone."""
    assert os.path.exists(SHIM), "shimccl.so not built (make -C tests)"
    env = dict(os.environ)
    pre = env.get("LD_PRELOAD")
    env["LD_PRELOAD"] = SHIM + (":" + pre if pre else "")
    env["SHIMCCL_DIR"] = str(tmp_path / "box")
    env.pop("HIP_VISIBLE_DEVICES", None)  # both ranks share device 0
    outs = [str(tmp_path / f"rank{r}.txt") for r in range(2)]
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(HERE, "dense_dist_worker.py"),
         str(r), outs[r]], env=env, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=120)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, log) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f"rank {r} failed:\n{log}"
    for r in range(2):
        got = open(outs[r]).read().split()
        assert got == [str(EARG)] * 6 + ["1"], f"rank {r}: {got}"


# ---------------- 7. conflux_amd.dense ---------------------------------------

def _dense_inputs(torch, n, kind):
    A = _mat(n)
    if kind == "row":
        return A, torch.from_numpy(A).cuda()
    if kind == "col":
        t = torch.from_numpy(A).cuda().T.contiguous().T
        assert t.stride() == (1, n)
        return A, t
    big = np.random.default_rng(n).standard_normal((2 * n, 2 * n))
    big[::2, ::2] = A
    t = torch.from_numpy(big).cuda()[::2, ::2]
    assert not t.is_contiguous()
    return A, t


@pytest.mark.parametrize("kind", ["row", "col", "slice"])
@pytest.mark.parametrize("n", [50, 300])
def test_dense_round_trip(torch, n, kind):
    from conflux_amd import dense
    A, tA = _dense_inputs(torch, n, kind)
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, 5))
    tB = torch.from_numpy(B).cuda()
    with dense.lu_factor(tA) as lu:
        assert lu.v == (128 if n == 300 else 32)
        X = lu.solve(tB)
        assert X.shape == tB.shape and X.data_ptr() != tB.data_ptr()
        assert np.array_equal(tB.cpu().numpy(), B), "solve changed B"
        _check_eta(A, X.cpu().numpy(), B, f"dense {kind} n={n}")
        _check_eta(A.T, lu.solve_transposed(tB).cpu().numpy(), B,
                   f"dense^T {kind} n={n}")
        x1 = lu.solve(tB[:, 0])  # 1-D, and a strided view of B
        assert x1.shape == (n,)
        _check_eta(A, x1.cpu().numpy()[:, None], B[:, :1],
                   f"dense 1-D {kind} n={n}")
        F, perm = lu.factors()
        assert F.shape == (n, n) and F.dtype == torch.float64
        assert perm.shape == (n,) and perm.dtype == torch.int32
        hF, hp = F.cpu().numpy(), perm.cpu().numpy()
        assert sorted(hp) == list(range(n))
        res = np.linalg.norm(A[hp] - (np.tril(hF, -1) + np.eye(n)) @
                             np.triu(hF)) / np.linalg.norm(A)
        assert res < 1e-14
        sg_np, ld_np = np.linalg.slogdet(A)
        sg, ld = lu.slogdet()
        assert sg == sg_np and abs(ld - ld_np) <= _logdet_tol(A, ld_np)
        assert 0 < lu.rcond("1") <= 1 and 0 < lu.rcond("I") <= 1
    with pytest.raises(ValueError):
        lu.solve(tB)  # closed


def test_dense_cholesky_and_nopivot(torch):
    from conflux_amd import dense
    n = 150
    S = _spd(n)
    tS = torch.from_numpy(S).cuda()
    b = np.random.default_rng(2).standard_normal(n)
    tb = torch.from_numpy(b).cuda()
    with dense.cholesky_factor(tS) as ch:
        assert ch.v == 64
        x = ch.solve(tb).cpu().numpy()
        _check_eta(S, x[:, None], b[:, None], "dense chol")
        ld_np = np.linalg.slogdet(S)[1]
        assert abs(ch.logdet() - ld_np) <= _logdet_tol(S, ld_np)
        assert 0 < ch.rcond() <= 1
    with dense.lu_factor(tS, v=32, pivot=False) as lu:
        _, perm = lu.factors()
        assert np.array_equal(perm.cpu().numpy(), np.arange(n))
        _check_eta(S, lu.solve(tb).cpu().numpy()[:, None], b[:, None],
                   "dense nopiv")
    with pytest.raises(ValueError):
        dense.lu_factor(tS.float())
    with pytest.raises(ValueError):
        dense.lu_factor(tS.cpu())
