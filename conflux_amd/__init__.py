"""conflux_amd — Python bindings for the MI355X-native CONFLUX LU engine.

The PRODUCT is the native library (libconflux_lu.so: C++ host + HIP/gfx950
kernels + RCCL) and the conflux_miniapp CLI.  This module is a thin ctypes
loader used by bench.py and the tests.  It FAILS LOUDLY if the HIP extension
is missing — there is no CPU fallback anywhere in the product path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libconflux_lu.so")

UID_BYTES = 128


class ConfluxLuError(RuntimeError):
    pass


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ConfluxLuError(
            f"HIP engine not built: {_LIB_PATH} missing. "
            "Run `make -C conflux_amd` (or __graft_entry__.build()). "
            "The product has no CPU fallback.")
    lib = ctypes.CDLL(_LIB_PATH)
    lib.conflux_lu_create.argtypes = [ctypes.c_int] * 7 + [
        ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.conflux_lu_make_uid.argtypes = [ctypes.c_char_p]
    lib.conflux_lu_init_matrix.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib.conflux_lu_init_matrix_spd.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib.conflux_chol_factor.argtypes = [ctypes.c_void_p,
                                        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_set_matrix_local.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_set_matrix_sim.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p]
    lib.conflux_lu_store_factors.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.conflux_lu_set_pivoting.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.conflux_lu_factor.argtypes = [ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_get_factors.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]
    lib.conflux_lu_get_factors_sim.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_dims.argtypes = [ctypes.c_void_p] + [
        ctypes.POINTER(ctypes.c_int)] * 6
    lib.conflux_lu_kernel_stats.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_validate.argtypes = [ctypes.c_void_p,
                                        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_chol_validate.argtypes = [ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_destroy.argtypes = [ctypes.c_void_p]
    lib.conflux_lu_build_info.restype = ctypes.c_char_p
    lib.conflux_lu_debug_dgemm.argtypes = [
        ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_debug_getrf.argtypes = [ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_debug_set_panel_glue.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_set_panel_reg.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_set_panel_publish.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_set_panel_phase_stats.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_panel_phase_stats.argtypes = [ctypes.c_void_p]
    lib.conflux_lu_debug_set_trsm_stripe.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_trsm_stripe_width.argtypes = []
    lib.conflux_lu_debug_trsm_ld.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
        ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p,
        ctypes.c_void_p]
    lib.conflux_lu_debug_set_one_rank_direct.argtypes = [ctypes.c_int]
    lib.conflux_lu_debug_trsm_oop.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong,
        ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_debug_dgemm_bench.argtypes = [
        ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_debug_trsm.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_solve.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_chol_solve.argtypes = lib.conflux_lu_solve.argtypes
    lib.conflux_lu_debug_trsm_left.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
        ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_debug_update_skinny.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_solve_refined.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_chol_solve_refined.argtypes = \
        lib.conflux_lu_solve_refined.argtypes
    lib.conflux_lu_debug_residual_dd.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.conflux_lu_debug_residual_group_width.argtypes = []
    lib.conflux_lu_debug_residual_dd_bench.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_solve_trans.argtypes = lib.conflux_lu_solve.argtypes
    lib.conflux_lu_rcond.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_chol_rcond.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_double)]
    lib.conflux_lu_debug_trsm_left_trans.argtypes = \
        lib.conflux_lu_debug_trsm_left.argtypes
    lib.conflux_lu_debug_update_skinny_t.argtypes = \
        lib.conflux_lu_debug_update_skinny.argtypes
    # kernel pins (whole host buffers up and down; EARG before any launch)
    i32, i64, ptr = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    lib.conflux_lu_debug_dgemm_ex.argtypes = [
        i32, i32, i32, i64, i32, i64, i64, i64, i64, ptr, ptr, ptr]
    lib.conflux_lu_debug_set_gemm_strip.argtypes = [i32]
    lib.conflux_lu_debug_set_gemm_ntc.argtypes = [i32]
    lib.conflux_lu_debug_dgemm_nt.argtypes = [
        i32, i64, i32, i64, i64, i64, i64, ptr, ptr, ptr,
        i32, i32, i64, i32, i32, i32, i32]
    lib.conflux_lu_debug_potrf32.argtypes = [i32, i64, i64, ptr]
    lib.conflux_lu_debug_getrf32_nopiv.argtypes = [i32, i64, i64, ptr]
    lib.conflux_lu_debug_trsm32.argtypes = [i32, i32, i64, i64, i64, ptr, ptr]
    lib.conflux_lu_debug_potrf_tile.argtypes = [i32, i64, i64, ptr]
    lib.conflux_lu_debug_poke_factor.argtypes = [ptr, i64, i64,
                                                 ctypes.c_double]
    # device-resident dense interface (ptr arguments are device addresses)
    dbl_p = ctypes.POINTER(ctypes.c_double)
    lib.conflux_lu_set_matrix_device.argtypes = [ptr, ptr, i64, i32, i32]
    lib.conflux_lu_get_factors_device.argtypes = [ptr, ptr, i64, ptr]
    lib.conflux_lu_solve_device.argtypes = [ptr, ptr, i64, i32, i32, dbl_p]
    lib.conflux_chol_solve_device.argtypes = [ptr, ptr, i64, i32, dbl_p]
    lib.conflux_lu_slogdet.argtypes = [ptr, dbl_p, dbl_p]
    lib.conflux_chol_logdet.argtypes = [ptr, dbl_p]
    lib.conflux_lu_logical_order.argtypes = [ptr, ctypes.POINTER(i32)]
    lib.conflux_lu_debug_get_input.argtypes = [ptr, i32, ptr]
    # refined solves: transposed, and on device buffers (berr/ferr are host)
    i32_p = ctypes.POINTER(i32)
    lib.conflux_lu_solve_refined_trans.argtypes = \
        lib.conflux_lu_solve_refined.argtypes
    lib.conflux_lu_solve_refined_device.argtypes = [
        ptr, ptr, i64, i32, i32, i32, ptr, ptr, i32_p, dbl_p]
    lib.conflux_chol_solve_refined_device.argtypes = [
        ptr, ptr, i64, i32, i32, ptr, ptr, i32_p, dbl_p]
    lib.conflux_lu_debug_residual_dd_t.argtypes = \
        lib.conflux_lu_debug_residual_dd.argtypes
    lib.conflux_lu_debug_residual_t_chunk.argtypes = []
    lib.conflux_lu_debug_residual_dd_t_bench.argtypes = [
        i32, i32, i32, i32, dbl_p, dbl_p, dbl_p]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _chk(rc, what):
    if rc != 0:
        raise ConfluxLuError(f"{what} failed: rc={rc}")


class Engine:
    """One factorization context.  rank=-1, world=P -> single-process
    multi-rank SIMULATION on one GPU (full choreography, D2D transport);
    rank>=0 -> one process per GPU over RCCL."""

    def __init__(self, N, v, Px, Py, Pz, rank=-1, world=None, uid=None):
        import numpy as np  # noqa: F401
        self.N, self.v, self.Px, self.Py, self.Pz = N, v, Px, Py, Pz
        P = Px * Py * Pz
        world = P if world is None else world
        self.world = world
        self.sim = rank < 0
        self._h = ctypes.c_void_p()
        _chk(lib().conflux_lu_create(N, v, Px, Py, Pz, rank, world, uid,
                                     ctypes.byref(self._h)), "create")
        d = [ctypes.c_int() for _ in range(6)]
        _chk(lib().conflux_lu_dims(self._h, *[ctypes.byref(x) for x in d]),
             "dims")
        self.Ml, self.Nl, self.Nt, self.nlayr, self.M, self.Npad = \
            (x.value for x in d)

    @staticmethod
    def make_uid():
        buf = ctypes.create_string_buffer(UID_BYTES)
        _chk(lib().conflux_lu_make_uid(buf), "make_uid")
        return buf.raw

    def init_matrix(self, seed=42):
        _chk(lib().conflux_lu_init_matrix(self._h, seed), "init_matrix")

    def set_matrix_global(self, A):
        """Distribute a full N x N numpy matrix (sim mode only)."""
        import numpy as np
        assert self.sim
        v = self.v
        for pi in range(self.Px):
            for pj in range(self.Py):
                loc = np.zeros((self.Ml, self.Nl))
                for lti in range(self.Ml // v):
                    for ltj in range(self.Nl // v):
                        gti, gtj = lti * self.Px + pi, ltj * self.Py + pj
                        loc[lti * v:(lti + 1) * v, ltj * v:(ltj + 1) * v] = \
                            A[gti * v:(gti + 1) * v, gtj * v:(gtj + 1) * v]
                loc = np.ascontiguousarray(loc)
                for pk in range(self.Pz):
                    g = (pi * self.Py + pj) * self.Pz + pk
                    buf = loc if pk == 0 else None
                    _chk(lib().conflux_lu_set_matrix_sim(
                        self._h, g,
                        buf.ctypes.data_as(ctypes.c_void_p) if buf is not None
                        else None), "set_matrix_sim")

    def set_matrix_local(self, local):
        ptr = None
        if local is not None:
            import numpy as np
            local = np.ascontiguousarray(local, dtype=np.float64)
            ptr = local.ctypes.data_as(ctypes.c_void_p)
        _chk(lib().conflux_lu_set_matrix_local(self._h, ptr), "set_matrix")

    def store_factors(self, enable):
        _chk(lib().conflux_lu_store_factors(self._h, int(enable)), "store")

    def set_pivoting(self, mode):
        """1 = tournament (default), 0 = none (EmptyPivot fast path for
        diagonally dominant inputs; perm stays identity)."""
        _chk(lib().conflux_lu_set_pivoting(self._h, int(mode)), "pivoting")

    def factor(self):
        ms = ctypes.c_double()
        _chk(lib().conflux_lu_factor(self._h, ctypes.byref(ms)), "factor")
        return ms.value

    def init_matrix_spd(self, seed=42):
        _chk(lib().conflux_lu_init_matrix_spd(self._h, seed), "init_spd")

    def factor_cholesky(self):
        ms = ctypes.c_double()
        _chk(lib().conflux_chol_factor(self._h, ctypes.byref(ms)), "chol")
        return ms.value

    def validate(self):
        """Device-side ||PA - LU||_F / ||A||_F of the last factorization
        (conflux_lu_validate; stripe-streamed).  COLLECTIVE when world > 1:
        every rank must call; all ranks return the broadcast residual."""
        r = ctypes.c_double()
        _chk(lib().conflux_lu_validate(self._h, ctypes.byref(r)), "validate")
        return r.value

    def validate_cholesky(self):
        """Device-side ||A - L L^T||_F / ||A||_F of the last Cholesky
        factorization.  COLLECTIVE when world > 1 (like validate)."""
        r = ctypes.c_double()
        _chk(lib().conflux_chol_validate(self._h, ctypes.byref(r)),
             "chol_validate")
        return r.value

    def _solve(self, fn, what, B, return_ms):
        import numpy as np
        B = np.asarray(B)
        if B.ndim not in (1, 2) or B.shape[0] != self.Npad:
            raise ValueError(
                f"{what}: B must be ({self.Npad},) or ({self.Npad}, nrhs), "
                f"got {B.shape}")
        X = np.array(B, dtype=np.float64, order="C")  # always a fresh copy
        nrhs = 1 if X.ndim == 1 else X.shape[1]
        ms = ctypes.c_double()
        _chk(fn(self._h, X.ctypes.data_as(ctypes.c_void_p), nrhs,
                ctypes.byref(ms)), what)
        return (X, ms.value) if return_ms else X

    def solve(self, B, return_ms=False):
        """Solve A X = B with the stored factors of the last factor()
        (store_factors on).  B: (Npad,) or (Npad, nrhs); returns a new array
        of the same shape, B itself is untouched.  return_ms=True also
        returns the device time of the two sweeps.  Single process only:
        a world > 1 engine raises ConfluxLuError (rc = EARG)."""
        return self._solve(lib().conflux_lu_solve, "solve", B, return_ms)

    def solve_cholesky(self, B, return_ms=False):
        """Solve L L^T X = B with the factor of the last factor_cholesky()
        (same conventions as solve)."""
        return self._solve(lib().conflux_chol_solve, "solve_cholesky", B,
                           return_ms)

    def solve_transposed(self, B, return_ms=False):
        """Solve A^T X = B with the stored factors of the last factor()
        (conflux_lu_solve_trans; same conventions as solve).  Raises
        ConfluxLuError after factor_cholesky(): there A = A^T and
        solve_cholesky is the answer."""
        return self._solve(lib().conflux_lu_solve_trans, "solve_transposed",
                           B, return_ms)

    def _rcond(self, what, call, return_info):
        rc = ctypes.c_double()
        an = ctypes.c_double()
        ns = ctypes.c_int()
        ms = ctypes.c_double()
        _chk(call(ctypes.byref(rc), ctypes.byref(an), ctypes.byref(ns),
                  ctypes.byref(ms)), what)
        if not return_info:
            return rc.value
        return rc.value, dict(anorm=an.value, nsolves=ns.value, ms=ms.value)

    def rcond(self, norm="1", return_info=False):
        """Estimate 1 / (||A|| ||A^-1||) of the (padded) matrix of the last
        factor() in the 1-norm (norm="1") or the infinity norm (norm="I")
        (conflux_lu_rcond: exact ||A||, Higham's estimator for ||A^-1||, so
        the result is an upper bound on the true rcond, usually tight).  0.0
        for a singular factorization.  return_info=True returns
        (rcond, info), info = dict(anorm=||A||, nsolves=single-RHS solves
        used, ms=device time of the estimation loop)."""
        if norm not in ("1", "I"):
            raise ValueError(f'rcond: norm must be "1" or "I", got {norm!r}')
        n = 0 if norm == "1" else 1
        return self._rcond(
            "rcond", lambda *a: lib().conflux_lu_rcond(self._h, n, *a),
            return_info)

    def rcond_cholesky(self, return_info=False):
        """rcond for the matrix of the last factor_cholesky() (symmetric:
        the two norms coincide).  Both triangles of the input must hold A."""
        return self._rcond(
            "rcond_cholesky",
            lambda *a: lib().conflux_chol_rcond(self._h, *a), return_info)

    def _solve_refined(self, fn, what, B, max_iter, return_info):
        import numpy as np
        B = np.asarray(B)
        if B.ndim not in (1, 2) or B.shape[0] != self.Npad:
            raise ValueError(
                f"{what}: B must be ({self.Npad},) or ({self.Npad}, nrhs), "
                f"got {B.shape}")
        X = np.array(B, dtype=np.float64, order="C")  # always a fresh copy
        nrhs = 1 if X.ndim == 1 else X.shape[1]
        berr = np.zeros(nrhs)
        ferr = np.zeros(nrhs)
        iters = ctypes.c_int()
        ms = ctypes.c_double()
        _chk(fn(self._h, X.ctypes.data_as(ctypes.c_void_p), nrhs,
                int(max_iter), berr.ctypes.data_as(ctypes.c_void_p),
                ferr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(iters),
                ctypes.byref(ms)), what)
        if not return_info:
            return X
        return X, dict(berr=berr, ferr=ferr, iters=iters.value, ms=ms.value)

    def solve_refined(self, B, max_iter=10, return_info=False):
        """solve() followed by up to max_iter passes of iterative refinement
        with a doubled-precision residual (conflux_lu_solve_refined): makes
        the no-pivot fast path backward stable on general input and recovers
        the digits an ill-conditioned system loses.  Same conventions as
        solve (B: (Npad,) or (Npad, nrhs), new array returned, B untouched);
        max_iter=0 is the plain solve plus its backward error.
        return_info=True returns (X, info), info = dict(berr=ndarray[nrhs]
        backward error of the returned X, ferr=ndarray[nrhs] last relative
        correction applied (an estimate, not a bound), iters=passes that
        applied a correction, ms=device time)."""
        return self._solve_refined(lib().conflux_lu_solve_refined,
                                   "solve_refined", B, max_iter, return_info)

    def solve_cholesky_refined(self, B, max_iter=10, return_info=False):
        """Refined solve on the factor of the last factor_cholesky() (same
        conventions as solve_refined).  The residual multiplies by the stored
        input as it stands: both of its triangles must hold A."""
        return self._solve_refined(lib().conflux_chol_solve_refined,
                                   "solve_cholesky_refined", B, max_iter,
                                   return_info)

    def solve_transposed_refined(self, B, max_iter=10, return_info=False):
        """solve_transposed() followed by up to max_iter passes of refinement
        (conflux_lu_solve_refined_trans; same conventions as solve_refined).
        The residual B - A^T X reads the stored input in place, berr takes
        ||A||1.  max_iter=0 is solve_transposed bit for bit.  Raises
        ConfluxLuError after factor_cholesky()."""
        return self._solve_refined(lib().conflux_lu_solve_refined_trans,
                                   "solve_transposed_refined", B, max_iter,
                                   return_info)

    # ---- device-resident dense interface --------------------------------
    # Pointers are raw device addresses (e.g. torch.Tensor.data_ptr()); the
    # caller owns the buffers and must have finished producing them — the
    # engine waits for its own stream only.  conflux_amd.dense wraps these
    # for torch tensors.

    @property
    def n(self):
        """Logical order of the current input: what set_matrix_device was
        given, Npad after every other way of setting the matrix."""
        n = ctypes.c_int()
        _chk(lib().conflux_lu_logical_order(self._h, ctypes.byref(n)),
             "logical_order")
        return n.value

    def set_matrix_device(self, dA, lda, n, order=0):
        """Import the caller's dense n x n device matrix (order 0: element
        (i, j) at dA[i*lda + j]; 1: dA[j*lda + i]) as blockdiag(A, I) of
        order Npad; 1 <= n <= Npad.  Single process only."""
        _chk(lib().conflux_lu_set_matrix_device(self._h, dA, lda, n, order),
             "set_matrix_device")

    def get_factors_device(self, dF, ldf, dperm):
        """Leading n x n block of the stored factors into the row-major
        device buffer dF (ldf >= n) and perm[:n] as int32 into dperm; either
        may be None."""
        _chk(lib().conflux_lu_get_factors_device(self._h, dF, ldf, dperm),
             "get_factors_device")

    def solve_device(self, dB, ldb, nrhs, trans=False):
        """Solve A X = B (A^T X = B with trans) in place on the device buffer
        dB (n x nrhs, row-major, ldb >= nrhs).  Returns the device time of
        the two sweeps in ms."""
        ms = ctypes.c_double()
        _chk(lib().conflux_lu_solve_device(self._h, dB, ldb, nrhs,
                                           int(bool(trans)),
                                           ctypes.byref(ms)), "solve_device")
        return ms.value

    def solve_cholesky_device(self, dB, ldb, nrhs):
        """solve_device for the factor of the last factor_cholesky()."""
        ms = ctypes.c_double()
        _chk(lib().conflux_chol_solve_device(self._h, dB, ldb, nrhs,
                                             ctypes.byref(ms)),
             "solve_cholesky_device")
        return ms.value

    def _refined_device(self, what, call, nrhs, max_iter):
        import numpy as np
        berr = np.zeros(max(int(nrhs), 0))
        ferr = np.zeros(max(int(nrhs), 0))
        iters = ctypes.c_int()
        ms = ctypes.c_double()
        _chk(call(int(max_iter), berr.ctypes.data_as(ctypes.c_void_p),
                  ferr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(iters),
                  ctypes.byref(ms)), what)
        return dict(berr=berr, ferr=ferr, iters=iters.value, ms=ms.value)

    def solve_refined_device(self, dB, ldb, nrhs, trans=False, max_iter=10):
        """solve_refined (solve_transposed_refined with trans) in place on the
        device buffer dB (n x nrhs, row-major, ldb >= nrhs; the slack is not
        touched).  Everything describes the n x n matrix of the logical
        order.  Returns the info dict of solve_refined: berr and ferr as
        numpy arrays, iters, ms."""
        return self._refined_device(
            "solve_refined_device",
            lambda *a: lib().conflux_lu_solve_refined_device(
                self._h, dB, ldb, nrhs, int(bool(trans)), *a),
            nrhs, max_iter)

    def solve_cholesky_refined_device(self, dB, ldb, nrhs, max_iter=10):
        """solve_refined_device for the factor of the last
        factor_cholesky(); both triangles of the input must hold A."""
        return self._refined_device(
            "solve_cholesky_refined_device",
            lambda *a: lib().conflux_chol_solve_refined_device(
                self._h, dB, ldb, nrhs, *a),
            nrhs, max_iter)

    def slogdet(self):
        """(sign, log|det A|) of the n x n matrix of the last factor(), like
        numpy.linalg.slogdet: (0.0, -inf) for a zero pivot."""
        sg = ctypes.c_double()
        ld = ctypes.c_double()
        _chk(lib().conflux_lu_slogdet(self._h, ctypes.byref(sg),
                                      ctypes.byref(ld)), "slogdet")
        return sg.value, ld.value

    def logdet_cholesky(self):
        """log det A = 2 sum log L_ii of the last factor_cholesky()."""
        ld = ctypes.c_double()
        _chk(lib().conflux_chol_logdet(self._h, ctypes.byref(ld)),
             "logdet_cholesky")
        return ld.value

    def get_perm(self):
        import numpy as np
        perm = np.zeros(self.M, dtype=np.int32)
        _chk(lib().conflux_lu_get_factors(self._h, None,
                                          perm.ctypes.data_as(ctypes.c_void_p)),
             "get_factors")
        return perm

    def get_F_global(self):
        """Assemble the global factored matrix F (pivoted rows) — sim mode."""
        import numpy as np
        assert self.sim
        v = self.v
        F = np.zeros((self.Npad, self.Npad))
        loc = np.zeros((self.Ml, self.Nl))
        for pi in range(self.Px):
            for pj in range(self.Py):
                g = (pi * self.Py + pj) * self.Pz + 0
                _chk(lib().conflux_lu_get_factors_sim(
                    self._h, g, loc.ctypes.data_as(ctypes.c_void_p), None),
                    "get_factors_sim")
                for lti in range(self.Ml // v):
                    for ltj in range(self.Nl // v):
                        gti, gtj = lti * self.Px + pi, ltj * self.Py + pj
                        F[gti * v:(gti + 1) * v, gtj * v:(gtj + 1) * v] = \
                            loc[lti * v:(lti + 1) * v, ltj * v:(ltj + 1) * v]
        return F

    def get_F_local(self):
        import numpy as np
        F = np.zeros((self.Ml, self.Nl))
        _chk(lib().conflux_lu_get_factors(self._h,
                                          F.ctypes.data_as(ctypes.c_void_p),
                                          None), "get_factors")
        return F

    def kernel_stats(self):
        out = {}
        names = {0: "dgemm_trailing", 1: "panel_getrf", 2: "trsm", 3: "rowmove"}
        for k, name in names.items():
            s = ctypes.c_double()
            n = ctypes.c_long()
            f = ctypes.c_double()
            _chk(lib().conflux_lu_kernel_stats(self._h, k, ctypes.byref(s),
                                               ctypes.byref(n),
                                               ctypes.byref(f)), "stats")
            out[name] = dict(seconds=s.value, launches=n.value, flops=f.value)
        return out

    def close(self):
        if self._h:
            lib().conflux_lu_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
