"""GPU parity tests: the HIP engine against the oracle (which is itself
pinned to the compiled reference — tests/test_oracle.py).

All tests run on ONE MI355X.  Multi-rank grids run in the engine's
single-process simulation mode: identical choreography and kernels as the
RCCL path, device-to-device transport.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import Params, gen_matrix, lu_oracle, residual_check  # noqa: E402
from _hp_ref import gemm_ratio  # noqa: E402

TOL_F = 1e-11
TOL_RES = 1e-14


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


# ---------------- kernel-level numerics (vs numpy fp64 reference) ----------

def test_dgemm_numerics(eng):
    rng = np.random.default_rng(0)
    for (M, N, K) in [(128, 128, 16), (256, 384, 32), (130, 257, 48),
                      (1, 128, 16), (300, 1, 512), (512, 512, 512)]:
        A = rng.standard_normal((M, K))
        B = rng.standard_normal((K, N))
        C = rng.standard_normal((M, N))
        C1 = C.copy()
        rc = eng.lib().conflux_lu_debug_dgemm(
            M, N, K, A.ctypes.data_as(ctypes.c_void_p),
            B.ctypes.data_as(ctypes.c_void_p),
            C1.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        # elementwise, against the longdouble reference and the derived
        # (K + 2) u (|A||B| + |C|) bound of tests/_hp_ref.py
        ratio = gemm_ratio(C1, A, B, C)
        assert ratio <= 1.0, f"dgemm M={M} N={N} K={K}: err/bound={ratio}"


def test_dgemm_transpose_detecting(eng):
    # asymmetric A and B catch any row/col swap in the MFMA C layout (G9)
    M = N = 64
    K = 16
    A = np.arange(M * K, dtype=np.float64).reshape(M, K) / 100
    B = (np.arange(K * N, dtype=np.float64).reshape(K, N) ** 1.5) / 1000
    C = np.zeros((M, N))
    C1 = C.copy()
    assert eng.lib().conflux_lu_debug_dgemm(
        M, N, K, A.ctypes.data_as(ctypes.c_void_p),
        B.ctypes.data_as(ctypes.c_void_p),
        C1.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.allclose(C1, -A @ B, atol=1e-10)


def test_getrf_matches_lapack(eng):
    import scipy.linalg as la
    rng = np.random.default_rng(1)
    for (n, v) in [(64, 32), (96, 32), (128, 64), (257, 64), (1024, 128)]:
        P0 = 5 + rng.random((n, v))
        P1 = P0.copy()  # debug_getrf factors in place — keep P0 pristine
        ipiv = np.zeros(v, dtype=np.int32)
        rc = eng.lib().conflux_lu_debug_getrf(
            n, v, P1.ctypes.data_as(ctypes.c_void_p),
            ipiv.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        lu, piv, info = la.lapack.dgetrf(np.asfortranarray(P0))
        nst = min(n, v)
        assert np.array_equal(ipiv[:nst], piv[:nst]), f"pivots n={n} v={v}"
        assert np.abs(P1 - lu).max() < 1e-12, f"factors n={n} v={v}"


def test_trsm_right_upper(eng):
    rng = np.random.default_rng(2)
    v, M = 64, 500
    U = np.triu(rng.random((v, v)) + np.eye(v) * 5)
    X = rng.standard_normal((M, v))
    X1 = X.copy()
    assert eng.lib().conflux_lu_debug_trsm(
        1, M, M, v, U.ctypes.data_as(ctypes.c_void_p),
        X1.ctypes.data_as(ctypes.c_void_p)) == 0
    ref = np.linalg.solve(U.T, X.T).T
    assert np.abs(X1 - ref).max() < 1e-12


def test_trsm_left_lower_unit(eng):
    rng = np.random.default_rng(3)
    v, N = 64, 700
    L = np.tril(rng.random((v, v)), -1) + np.eye(v)
    X = rng.standard_normal((v, N))
    X1 = X.copy()
    assert eng.lib().conflux_lu_debug_trsm(
        0, v, N, v, L.ctypes.data_as(ctypes.c_void_p),
        X1.ctypes.data_as(ctypes.c_void_p)) == 0
    ref = np.linalg.solve(L, X)
    assert np.abs(X1 - ref).max() < 1e-12


# ---------------- end-to-end parity vs the oracle ---------------------------

GRIDS = [
    (64, 8, 1, 1, 1),
    (128, 16, 1, 1, 1),
    (128, 16, 1, 1, 2),
    (64, 8, 2, 2, 1),
    (64, 8, 2, 2, 2),
    (128, 16, 2, 2, 2),
    (128, 8, 4, 4, 2),
    (256, 32, 2, 2, 1),
    (512, 32, 8, 8, 1),   # 3-round butterfly (ceil(log2 8)); Ml = 2v edge
]


@pytest.mark.parametrize("N,v,Px,Py,Pz", GRIDS)
def test_lu_parity(eng, N, v, Px, Py, Pz):
    A = gen_matrix(N)
    p = Params(N, v, Px, Py, Pz)
    r = lu_oracle(A, p)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, r["perm"]), "pivot indices must be bit-exact"
    assert np.abs(F - r["F"]).max() < TOL_F
    assert residual_check(A, perm, F) < TOL_RES


def test_lu_parity_golden(eng, golden):
    """Engine vs the compiled reference's own outputs (golden fixtures)."""
    checked = 0
    for tag in sorted({k.split("/")[0] for k in golden.files}):
        N, v, Px, Py, Pz = (int(x) for x in golden[f"{tag}/cfg"])
        if N > 256:
            continue
        A = golden[f"{tag}/A"]
        with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
            e.store_factors(True)
            e.set_matrix_global(A)
            e.factor()
            perm = e.get_perm()
            F = e.get_F_global()
        assert np.array_equal(perm, golden[f"{tag}/perm"]), f"{tag} pivots"
        assert np.abs(F - golden[f"{tag}/C"]).max() < TOL_F, f"{tag} factors"
        checked += 1
    assert checked >= 8


@pytest.mark.parametrize("N,v", [(1024, 128), (2048, 256)])
def test_lu_single_rank_medium(eng, N, v):
    """Size-scaling property check at sizes the oracle still runs fast."""
    A = gen_matrix(N)
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    # size-independent property: ||PA - LU||/||A|| at fp64
    assert residual_check(A, perm, F) < 1e-13
    # pivots vs LAPACK partial pivoting (1x1x1 degenerates to getrf)
    import scipy.linalg as la
    lu, piv = la.lu_factor(A)
    ref = np.arange(N)
    for i, j in enumerate(piv):
        ref[i], ref[j] = ref[j], ref[i]
    assert np.array_equal(perm, ref)



@pytest.mark.parametrize("N,v,Px,Py,Pz", [(256, 64, 1, 1, 1), (512, 64, 2, 2, 1)])
def test_lu_validate_device(eng, N, v, Px, Py, Pz):
    """conflux_lu_validate (device-side ||PA-LU||_F/||A||_F)
    agrees with the numpy residual computed from the gathered factors."""
    A = gen_matrix(N)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
        r_dev = e.validate()
    L = np.tril(F, -1) + np.eye(N)
    U = np.triu(F)
    r_np = np.linalg.norm(A[perm] - L @ U) / np.linalg.norm(A)
    assert r_dev < 1e-13
    assert abs(r_dev - r_np) < 1e-15 + 0.05 * r_np


def test_lu_zero_pivot_column(eng):
    """Singular input (a zero column, placed in the LAST tile column —
    see tests/test_oracle.py for why): the engine must follow LAPACK's
    zero-pivot convention (no scaling, factorization continues) and stay
    bit-exact with the oracle's pivot sequence."""
    N, v = 128, 64
    A = gen_matrix(N)
    A[:, 96] = 0.0
    p = Params(N, v, 1, 1, 1)
    r = lu_oracle(A, p)
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, r["perm"])
    assert np.allclose(F, r["F"], atol=1e-11, rtol=0)


def test_lu_factor_preserves_input(eng):
    """factor() factors a COPY of the uploaded matrix (the reference's
    LU_rep does not clobber lu_params::data, conflux_opt.hpp:398): a second
    factor() without re-upload must reproduce the first result exactly."""
    N, v = 256, 64
    A = gen_matrix(N)
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm1 = e.get_perm().copy()
        F1 = e.get_F_global().copy()
        e.factor()  # no re-upload
        perm2 = e.get_perm()
        F2 = e.get_F_global()
    assert np.array_equal(perm1, perm2)
    assert np.array_equal(F1, F2)


# ---------------- Cholesky (CONFCHOX path) ---------------------


@pytest.mark.parametrize("N,v,Px,Py,Pz", [(256, 64, 1, 1, 1), (512, 64, 2, 2, 1)])
def test_chol_validate_device(eng, N, v, Px, Py, Pz):
    """conflux_chol_validate agrees with the numpy residual."""
    A = _spd(N)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor_cholesky()
        F = e.get_F_global()
        r_dev = e.validate_cholesky()
    L = np.tril(F)
    r_np = np.linalg.norm(A - L @ L.T) / np.linalg.norm(A)
    assert r_dev < 1e-13
    assert abs(r_dev - r_np) < 1e-15 + 0.05 * r_np


def _spd(N):
    G = gen_matrix(N)
    return 0.5 * (G + G.T) + 2.0 * N * np.eye(N)


CHOL_GRIDS = [
    (64, 8, 1, 1, 1),
    (128, 16, 1, 1, 2),
    (128, 16, 2, 2, 1),
    (128, 16, 2, 2, 2),
    (128, 8, 4, 4, 2),
    (256, 32, 2, 2, 2),
    (96, 32, 1, 1, 1),    # odd tile count (Nt=3)
    (192, 32, 2, 2, 2),   # odd tiles per rank row
    (96, 8, 1, 1, 4),     # nlayr = 2
]


@pytest.mark.parametrize("N,v,Px,Py,Pz", CHOL_GRIDS)
def test_cholesky_parity(eng, N, v, Px, Py, Pz):
    """Engine Cholesky vs scipy/LAPACK dpotrf on the same SPD input.
    Pivotless path: no discrete choices, so LAPACK is the oracle."""
    import scipy.linalg as la
    A = _spd(N)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor_cholesky()
        F = e.get_F_global()
    L = np.tril(F)
    Lref = la.cholesky(A, lower=True)
    assert np.abs(L - Lref).max() < 1e-9 * N
    res = np.linalg.norm(A - L @ L.T) / np.linalg.norm(A)
    assert res < 1e-14


def test_cholesky_device_spd_generator(eng):
    """init_matrix_spd (device) must realize the same SPD matrix as the
    host formula: factor it and compare L against scipy of the host A."""
    import scipy.linalg as la
    N, v = 128, 16
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        import conflux_amd, ctypes
        conflux_amd.lib().conflux_lu_init_matrix_spd(e._h, 42)
        e.factor_cholesky()
        F = e.get_F_global()
    Lref = la.cholesky(_spd(N), lower=True)
    assert np.abs(np.tril(F) - Lref).max() < 1e-10


def test_cholesky_residual_medium(eng):
    N, v = 1024, 128
    A = _spd(N)
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor_cholesky()
        F = e.get_F_global()
    L = np.tril(F)
    assert np.linalg.norm(A - L @ L.T) / np.linalg.norm(A) < 1e-14


def test_cholesky_parity_reference_golden(eng):
    """Engine Cholesky on the reference CONFCHOX's OWN generated inputs vs
    the reference's own factored output (tests/golden/chol_golden.npz,
    captured from the DEBUG dumps of the compiled reference miniapp)."""
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "chol_golden.npz")
    if not os.path.exists(path):
        pytest.skip("chol_golden.npz missing")
    g = np.load(path)
    checked = 0
    for tag in sorted({k.split("/")[0] for k in g.files}):
        N, v, Px, Py, Pz = (int(x) for x in g[f"{tag}/cfg"])
        A = g[f"{tag}/A"]       # raw reference dump: lower triangle valid
        Lref = g[f"{tag}/L"]
        with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
            e.store_factors(True)
            e.set_matrix_global(A)  # engine also reads the lower half only
            e.factor_cholesky()
            F = e.get_F_global()
        assert np.abs(np.tril(F) - Lref).max() < 1e-10, f"{tag}"
        checked += 1
    assert checked >= 3


# ---------------- drop-in CLI (the §8b boundary) ----------------------------

def _repo_root():
    import os
    return os.path.join(os.path.dirname(__file__), "..")


def test_miniapp_cli_lu():
    """conflux_miniapp drop-in CLI: reference flags, _result_ contract line
    (conflux_miniapp.cpp:119,156-165) and the validation residual."""
    import os
    import re
    import subprocess
    out = subprocess.run(
        [os.path.join(_repo_root(), "conflux_amd", "conflux_miniapp"),
         "-N", "512", "-b", "64", "--p_grid=2,2,1", "--sim", "-r", "1"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    m = re.search(r"_result_ lu,conflux,512,512,4,2x2x1,time,other,\d+,64",
                  out.stdout)
    assert m, out.stdout
    r = re.search(r"relative residual \|\|PA-LU\|\|_F/\|\|A\|\|_F = ([0-9.e+-]+)",
                  out.stdout)
    assert r and float(r.group(1)) < 1e-13, out.stdout


def test_miniapp_cli_cholesky():
    import os
    import re
    import subprocess
    out = subprocess.run(
        [os.path.join(_repo_root(), "conflux_amd", "cholesky_miniapp"),
         "--dim", "512", "--tile", "64", "--grid", "2,2,1", "--sim",
         "--run", "1"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert re.search(r"_result_ chol,conflux,512,4,2x2x1,time,\d+,64",
                     out.stdout), out.stdout
    r = re.search(
        r"relative residual \|\|A-LL\^T\|\|_F/\|\|A\|\|_F = ([0-9.e+-]+)",
        out.stdout)
    assert r and float(r.group(1)) < 1e-13, out.stdout


@pytest.mark.timeout(600)
def test_miniapp_cli_full_cfg4_single_gpu():
    """Regression for the silent 2^32-thread launch rejection: at N=65536
    a flat per-element launch needs exactly 2^32 threads, one past HIP's
    limit — the init kernel was rejected silently and LU factored a zero
    matrix into NaNs.  The grid-stride kernels must handle the full cfg-4
    size on one GPU (it fits: ~70 GB of 288 GB HBM)."""
    import os
    import re
    import subprocess
    out = subprocess.run(
        [os.path.join(_repo_root(), "conflux_amd", "conflux_miniapp"),
         "-N", "65536", "-b", "512", "--p_grid=1,1,1", "-r", "1",
         "--timing"],
        capture_output=True, text=True, timeout=550)
    assert out.returncode == 0, (out.stdout, out.stderr)
    m = re.search(r"_result_ lu,conflux,65536,65536,1,1x1x1,time,other,(\d+),512",
                  out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) < 60000  # sanity: minutes would mean spin stalls


@pytest.mark.parametrize("seed", [7, 1234, 987654321])
def test_lu_parity_seeds(eng, seed):
    """Seed fuzz: the device generator and the whole pipeline stay
    pivot-bit-exact vs the oracle on inputs other than the bench seed."""
    N, v, Px, Py, Pz = 256, 32, 2, 2, 1
    A = gen_matrix(N, seed)
    r = lu_oracle(A, Params(N, v, Px, Py, Pz))
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.init_matrix(seed)            # device-side generator, same seed
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, r["perm"])
    assert np.abs(F - r["F"]).max() < TOL_F
    assert residual_check(A, perm, F) < TOL_RES


def test_lu_parity_8192_tournament(eng):
    """Bit-exact pivot ceiling at the bench tile size: N=8192, v=512,
    2x2x1 — tournament pivoting over 2 rank rows at real panel widths
    (the largest size the oracle restatement runs in about a minute)."""
    N, v = 8192, 512
    A = gen_matrix(N)
    r = lu_oracle(A, Params(N, v, 2, 2, 1))
    with eng.Engine(N, v, 2, 2, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, r["perm"]), "pivots bit-exact at N=8192"
    assert np.abs(F - r["F"]).max() < 1e-9
    assert residual_check(A, perm, F) < 1e-13


@pytest.mark.parametrize("N,v,Px,Py,Pz", [
    (96, 32, 1, 1, 1),    # odd tile count (Nt=3)
    (224, 32, 1, 1, 2),   # odd Nt=7 with depth replication
    (192, 32, 2, 2, 1),   # Nt=6: odd tiles per rank row (3)
    (192, 32, 2, 2, 2),   # same with Pz
    (96, 8, 1, 1, 4),     # nlayr = v/Pz = 2 (deep replication, tiny slabs)
    (160, 16, 2, 2, 2),   # Nt=10, small v
    (384, 64, 2, 2, 4),   # v=64 split 4 ways (nlayr=16)
])
def test_lu_parity_envelope_corners(eng, N, v, Px, Py, Pz):
    """Envelope corners the main GRIDS list misses: odd global tile counts,
    odd tiles-per-rank, deep Pz splits with tiny nlayr slabs."""
    A = gen_matrix(N)
    r = lu_oracle(A, Params(N, v, Px, Py, Pz))
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, r["perm"])
    assert np.abs(F - r["F"]).max() < TOL_F
    assert residual_check(A, perm, F) < TOL_RES


def test_lu_parity_bench_size(eng):
    """Pivots bit-exact vs the oracle restatement at the FULL bench size
    (N=16384, v=512) — the oracle runs in ~25 s on the GPU box's host
    cores, so the headline configuration itself is pivot-pinned every
    round, not just residual-checked."""
    N, v = 16384, 512
    A = gen_matrix(N)
    ref = lu_oracle(A, Params(N, v, 1, 1, 1))
    with eng.Engine(N, v, 1, 1, 1, rank=-1) as e:
        e.store_factors(True)
        e.set_matrix_global(A)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
    assert np.array_equal(perm, ref["perm"]), "bench-size pivots"
    assert np.abs(F - ref["F"]).max() < 1e-8
    assert residual_check(A, perm, F) < 1e-13


# ---------------- no-pivot fast path (EmptyPivot) -------------

@pytest.mark.parametrize("N,v,Px,Py,Pz", [
    (256, 64, 1, 1, 1),
    (256, 64, 2, 2, 1),
    (256, 64, 2, 2, 2),
    (512, 128, 2, 2, 1),
])
def test_lu_nopivot_parity(eng, N, v, Px, Py, Pz):
    """conflux_lu_set_pivoting(ctx, 0): the EmptyPivot fast path on a
    diagonally dominant input, vs the numpy no-pivot restatement; identity
    permutation and the unchanged device residual."""
    from oracle import lu_nopivot
    A = gen_matrix(N)
    S = 0.5 * (A + A.T) + 2.0 * N * np.eye(N)  # == init_matrix_spd fill
    ref = lu_nopivot(S, v)
    with eng.Engine(N, v, Px, Py, Pz, rank=-1) as e:
        e.store_factors(True)
        e.set_pivoting(0)
        e.set_matrix_global(S)
        e.factor()
        perm = e.get_perm()
        F = e.get_F_global()
        resid = e.validate()
    assert np.array_equal(perm, np.arange(N))
    scale = np.abs(ref).max()
    assert np.abs(F - ref).max() < 1e-11 * scale
    assert resid < 1e-14
