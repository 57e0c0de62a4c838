"""conflux_amd.dense — factor and solve a dense float64 torch device tensor.

    import torch
    from conflux_amd import dense
    A = torch.randn(1000, 1000, dtype=torch.float64, device="cuda")
    B = torch.randn(1000, 4, dtype=torch.float64, device="cuda")
    with dense.lu_factor(A) as lu:
        X = lu.solve(B)
        sign, logabsdet = lu.slogdet()

The matrix never leaves the device and needs no padding or re-tiling by the
caller: the engine imports it as blockdiag(A, I) of its own padded order
(conflux_lu_set_matrix_device) and every answer is about the n x n A.  One
GPU, one process (the one-rank engine).  There is no fallback: a missing
native library raises ConfluxLuError on first use.

Fast and accurate: the no-pivot factorization is the engine's fastest path,
and refinement makes it backward stable on general input —

    with dense.lu_factor(A, pivot=False) as lu:
        X, info = lu.solve(B, refine=True, return_info=True)
        assert (info["berr"] < 1e-15).all()

pivot=False WITHOUT refine is for diagonally dominant A only: on general
input the unpivoted elimination leaves a backward error of 1e-13 ... 1e-11.
refine works on solve, solve_transposed and Cholesky.solve alike, and costs
one pass over A plus one more solve per refinement pass.

Tile size: v=None picks the largest of 512/256/128/64/32 with 2 v <= n — the
engine needs at least two tiles per side (Ml >= 2 v) and larger tiles factor
faster.  Below n = 64 it is 32 and the engine pads n up to 64.

Import order: this module imports torch when it is imported.  A torch wheel
that bundles its own HIP runtime has to load it BEFORE the engine's library
is loaded (the engine then binds to that same copy); the other way round the
process holds two HIP runtimes and torch finds no GPU.  So import torch, or
this module, before the first conflux_amd.Engine / conflux_amd.lib() call
of the process.  A torch built against the system ROCm has no such
constraint.

Streams: the engine works on a stream of its own and waits only for that
one, so each call first synchronizes torch's current stream (the tensors
handed in are then complete) and returns with its results complete.
"""
import torch

from . import Engine

_V_CHOICES = (512, 256, 128, 64, 32)


def default_v(n):
    """Largest of 512/256/128/64/32 with 2 v <= n, else 32."""
    for v in _V_CHOICES:
        if 2 * v <= n:
            return v
    return 32


def _torch():
    return torch


def _check_matrix(A):
    torch = _torch()
    if not isinstance(A, torch.Tensor) or A.dim() != 2 or \
            A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError("A must be a square 2-D tensor")
    if A.dtype != torch.float64:
        raise ValueError(f"A must be float64, got {A.dtype}")
    if not A.is_cuda:
        raise ValueError("A must be a device tensor")


def _layout(A):
    """(tensor to pass, lda, order) by stride inspection: a row-major or a
    column-major A (unit stride along one index, leading dimension >= n along
    the other) passes as it is; anything else is made contiguous."""
    n = A.shape[0]
    s0, s1 = A.stride()
    if s1 == 1 and s0 >= n:
        return A, s0, 0
    if s0 == 1 and s1 >= n:
        return A, s1, 1
    if n == 1:
        return A, 1, 0
    A = A.contiguous()
    return A, n, 0


def _max_iter(refine):
    """refine keyword -> the engine's max_iter: False/0 off, True 10, a
    positive int itself."""
    if refine is True:
        return 10
    if refine is False or refine is None:
        return 0
    if not isinstance(refine, int):
        raise ValueError(f"refine must be a bool or an int, got {refine!r}")
    if refine < 0:
        raise ValueError(f"refine must be >= 0, got {refine}")
    return refine


class _Factored:
    """Shared part of LU and Cholesky: owns the engine, stages B."""

    def __init__(self, A, v):
        _check_matrix(A)
        torch = _torch()
        self.n = A.shape[0]
        self.v = default_v(self.n) if v is None else int(v)
        self.device = A.device
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            self._e = Engine(max(self.n, 2 * self.v), self.v, 1, 1, 1,
                             rank=0, world=1)
            try:
                self._e.store_factors(True)
                src, lda, order = _layout(A)
                self._e.set_matrix_device(src.data_ptr(), lda, self.n, order)
            except Exception:
                self.close()
                raise

    def _engine(self):
        if self._e is None:
            raise ValueError("factorization is closed")
        return self._e

    def _solve(self, B, call, refined, refine=False, return_info=False):
        """call(e, ptr, ld, nrhs) is the plain device solve, refined(e, ptr,
        ld, nrhs, max_iter) the refined one (returns the engine's info
        dict).  The plain call serves unless refinement or its figures are
        asked for."""
        torch = _torch()
        max_iter = _max_iter(refine)
        if not isinstance(B, torch.Tensor) or B.dim() not in (1, 2) or \
                B.shape[0] != self.n:
            raise ValueError(f"B must be ({self.n},) or ({self.n}, nrhs)")
        if B.dtype != torch.float64 or B.device != self.device:
            raise ValueError("B must be float64 on the matrix's device")
        e = self._engine()
        X = B.reshape(self.n, -1).clone(memory_format=torch.contiguous_format)
        nrhs = X.shape[1]
        info = dict(berr=torch.zeros(nrhs, dtype=torch.float64),
                    ferr=torch.zeros(nrhs, dtype=torch.float64), iters=0)
        if nrhs > 0:
            with torch.cuda.device(self.device):
                torch.cuda.current_stream().synchronize()
                if max_iter == 0 and not return_info:
                    call(e, X.data_ptr(), nrhs, nrhs)
                else:
                    raw = refined(e, X.data_ptr(), nrhs, nrhs, max_iter)
                    info = dict(berr=torch.from_numpy(raw["berr"]),
                                ferr=torch.from_numpy(raw["ferr"]),
                                iters=int(raw["iters"]))
        X = X.reshape(B.shape)
        return (X, info) if return_info else X

    def close(self):
        if getattr(self, "_e", None) is not None:
            self._e.close()
            self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LU(_Factored):
    """P A = L U of a dense device matrix, kept in the engine."""

    def __init__(self, A, v=None, pivot=True):
        super().__init__(A, v)
        try:
            self._e.set_pivoting(1 if pivot else 0)
            self._e.factor()
        except Exception:
            self.close()
            raise

    def solve(self, B, refine=False, return_info=False):
        """X with A X = B; B is (n,) or (n, nrhs) and is left untouched.
        refine: False / 0 the plain solve; True up to 10 passes of iterative
        refinement with a doubled-precision residual, a positive int that
        many; negative raises ValueError.  return_info=True returns
        (X, info): info["berr"] / info["ferr"] float64 CPU tensors of shape
        (nrhs,) — backward error of the returned X in the inf-norm of the
        n x n A, and the last relative correction applied — and
        info["iters"], the passes that applied one."""
        return self._solve(
            B, lambda e, p, ld, k: e.solve_device(p, ld, k),
            lambda e, p, ld, k, it: e.solve_refined_device(
                p, ld, k, max_iter=it), refine, return_info)

    def solve_transposed(self, B, refine=False, return_info=False):
        """X with A^T X = B (same conventions as solve; berr in the inf-norm
        of A^T)."""
        return self._solve(
            B, lambda e, p, ld, k: e.solve_device(p, ld, k, trans=True),
            lambda e, p, ld, k, it: e.solve_refined_device(
                p, ld, k, trans=True, max_iter=it), refine, return_info)

    def slogdet(self):
        """(sign, log|det A|) as Python floats, like numpy.linalg.slogdet."""
        return self._engine().slogdet()

    def rcond(self, norm="1"):
        """Estimate of 1 / (||A|| ||A^-1||) of the n x n A, norm "1" or
        "I"."""
        return self._engine().rcond(norm)

    def factors(self):
        """(LU, perm): the packed factors as an (n, n) float64 tensor (strict
        lower = L with unit diagonal, upper = U) and perm as an (n,) int32
        tensor, row r of P A being row perm[r] of A."""
        torch = _torch()
        e = self._engine()
        F = torch.empty((self.n, self.n), dtype=torch.float64,
                        device=self.device)
        perm = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            e.get_factors_device(F.data_ptr(), self.n, perm.data_ptr())
        return F, perm


class Cholesky(_Factored):
    """A = L L^T of a dense SPD device matrix (both triangles must hold A)."""

    def __init__(self, A, v=None):
        super().__init__(A, v)
        try:
            self._e.factor_cholesky()
        except Exception:
            self.close()
            raise

    def solve(self, B, refine=False, return_info=False):
        """X with A X = B; B is (n,) or (n, nrhs) and is left untouched.
        refine and return_info as for LU.solve."""
        return self._solve(
            B, lambda e, p, ld, k: e.solve_cholesky_device(p, ld, k),
            lambda e, p, ld, k, it: e.solve_cholesky_refined_device(
                p, ld, k, max_iter=it), refine, return_info)

    def logdet(self):
        """log det A as a Python float."""
        return self._engine().logdet_cholesky()

    def rcond(self):
        """Estimate of 1 / (||A|| ||A^-1||) of the n x n A."""
        return self._engine().rcond_cholesky()


def lu_factor(A, v=None, pivot=True):
    """Factor the 2-D float64 device tensor A (n x n, any n >= 1) and return
    an LU object.  A row-major or column-major A is read where it lies; any
    other striding is copied once.  v: tile size, default default_v(n);
    pivot=False takes the engine's no-pivot path (diagonally dominant A)."""
    return LU(A, v=v, pivot=pivot)


def cholesky_factor(A, v=None):
    """Cholesky-factor the SPD float64 device tensor A; returns an object
    with .solve, .logdet and .rcond."""
    return Cholesky(A, v=v)


__all__ = ["lu_factor", "cholesky_factor", "LU", "Cholesky", "default_v"]
