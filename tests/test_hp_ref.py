"""The bounds of tests/_hp_ref.py hold for a correct kernel and reject a
subtly wrong one: each kernel is emulated in fp64 numpy in its own operation
order and must stay inside its bound (a), and one planted defect of each kind
must land far outside it (b).  No GPU: this is the evidence that the GPU pins
would fail on a wrong kernel."""
import numpy as np
import pytest

import _hp_ref as hp

GEMM_SHAPES = [(1, 1, 1), (129, 257, 17), (300, 1, 512), (1, 130, 15),
               (128, 128, 16), (385, 1153, 40), (257, 1409, 16)]
NT_SHAPES = [(1, 1, 1), (129, 257, 17), (300, 130, 8)]
FAR = 1e6          # a defect must exceed its bound by at least this factor


def _gemm_inputs(seed, M, N, K, nt=False):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((N, K) if nt else (K, N))
    C = rng.standard_normal((M, N))
    return A, B, C


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_emulation_inside_bound(M, N, K):
    A, B, C = _gemm_inputs(1, M, N, K)
    assert hp.gemm_ratio(hp.emu_gemm(A, B, C), A, B, C) <= 1.0
    # numpy's own product (another summation order) is inside it too
    assert hp.gemm_ratio(C - A @ B, A, B, C) <= 1.0


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_emulation_inside_bound(M, N, K):
    A, B, C = _gemm_inputs(2, M, N, K, nt=True)
    assert hp.gemm_ratio(hp.emu_gemm(A, B, C, nt=True), A, B, C, nt=True) <= 1.0


def test_gemm_exact_case_is_exact():
    rng = np.random.default_rng(3)
    A, B, C = hp.ints(rng, (129, 17)), hp.ints(rng, (17, 257)), \
        hp.ints(rng, (129, 257))
    assert hp.bits_equal(hp.emu_gemm(A, B, C), hp.gemm_exact(A, B, C))
    bad = hp.emu_gemm(A, B, C, drop=(5, 7, 3))
    if A[5, 3] * B[3, 7] != 0:
        assert not hp.bits_equal(bad, hp.gemm_exact(A, B, C))


@pytest.mark.parametrize("M,N,K", [(129, 257, 17), (385, 1153, 40),
                                   (300, 1, 512)])
def test_gemm_dropped_term_rejected(M, N, K):
    A, B, C = _gemm_inputs(4, M, N, K)
    i, j, k = M - 1, N - 1, K - 1          # the last term of a corner element
    bad = hp.emu_gemm(A, B, C, drop=(i, j, k))
    assert hp.gemm_ratio(bad, A, B, C) > FAR


def test_gemm_nt_transposed_element_rejected():
    A, B, C = _gemm_inputs(5, 64, 64, 32, nt=True)
    bad = hp.emu_gemm(A, B, C, nt=True, swap=(3, 5))
    assert hp.gemm_ratio(bad, A, B, C, nt=True) > FAR


MASKS = [(128, 384, 512, 64, r0, c0, g)
         for r0 in (0, 128) for c0 in (0, 256)
         for g in [(1, 1, 0, 0), (2, 2, 0, 1), (2, 2, 1, 0), (2, 2, 1, 1),
                   (4, 4, 3, 0)]] + [(256, 512, 512, 128, 0, 0, (2, 2, 1, 0))]


# the one set of the list that the rule puts wholly above the tile diagonal
# (global tile rows 0, 2, 4 against tile columns 5, 7, 9, 11): nothing may
# be written there at all
ALL_MASKED = (128, 384, 512, 64, 0, 256, (2, 2, 0, 1))


@pytest.mark.parametrize("v,M,N,K,r0off,c0off,grid", MASKS)
def test_mask_sets_are_mixed(v, M, N, K, r0off, c0off, grid):
    upd = hp.tri_mask(M, N, v, r0off, c0off, *grid)
    assert not upd.all()
    assert upd.any() != ((v, M, N, K, r0off, c0off, grid) == ALL_MASKED)


def test_masked_nt_flipped_tile_rejected():
    v, M, N, K = 128, 384, 512, 64
    A, B, C = _gemm_inputs(6, M, N, K, nt=True)
    upd = hp.tri_mask(M, N, v, 0, 0, 2, 2, 1, 0)
    ratio, same = hp.masked_nt_check(hp.emu_masked_nt(A, B, C, upd), A, B, C,
                                     upd)
    assert ratio <= 1.0 and same
    on = np.argwhere(upd)[0]
    off = np.argwhere(~upd)[0]
    skipped = upd.copy()
    skipped[tuple(on)] = False             # a tile that should run does not
    ratio, same = hp.masked_nt_check(hp.emu_masked_nt(A, B, C, skipped), A, B,
                                     C, upd)
    assert ratio > FAR
    extra = upd.copy()
    extra[tuple(off)] = True               # a tile above the diagonal runs
    ratio, same = hp.masked_nt_check(hp.emu_masked_nt(A, B, C, extra), A, B,
                                     C, upd)
    assert not same


@pytest.mark.parametrize("nb", [1, 7, 16, 31, 32])
def test_potrf32_emulation(nb):
    rng = np.random.default_rng(10 + nb)
    A = hp.spd(rng, nb)
    F = hp.emu_potrf32(A)
    assert hp.potrf_ratio(A, F) <= 1.0
    assert hp.bits_equal(np.triu(F, 1), np.triu(A, 1))
    L0 = hp.exact_lower(rng, nb)
    assert hp.bits_equal(np.tril(hp.emu_potrf32(L0 @ L0.T)), L0)
    if nb >= 7:                            # one trailing update left out
        bad = F.copy()
        bad[nb - 1, nb - 2] = (A[nb - 1, nb - 2]
                               - F[nb - 1, :nb - 3] @ F[nb - 2, :nb - 3]
                               ) / F[nb - 2, nb - 2]
        assert hp.potrf_ratio(A, bad) > FAR


@pytest.mark.parametrize("nb", [1, 7, 16, 31, 32])
def test_getrf32_nopiv_emulation(nb):
    rng = np.random.default_rng(20 + nb)
    A = hp.diag_dominant(rng, nb)
    F = hp.emu_getrf32_nopiv(A)
    assert hp.getrf_ratio(A, F) <= 1.0
    L0, U0 = hp.exact_lower(rng, nb, unit=True), hp.exact_upper(rng, nb)
    assert hp.bits_equal(hp.emu_getrf32_nopiv(L0 @ U0),
                         np.tril(L0, -1) + U0)
    if nb >= 7:                            # element taken from the transpose
        bad = F.copy()
        bad[nb - 1, 2] = F[2, nb - 1]
        assert hp.getrf_ratio(A, bad) > FAR


def test_getrf32_nopiv_zero_pivot_emulation():
    rng = np.random.default_rng(30)
    A = hp.diag_dominant(rng, 16)
    A[:, 0] = 0.0
    F = hp.emu_getrf32_nopiv(A)
    assert np.isfinite(F).all() and (F[:, 0] == 0).all()
    assert hp.getrf_ratio(A, F) <= 1.0


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("nb", [1, 7, 32])
def test_trsm32_emulation(trans, nb):
    rng = np.random.default_rng(40 + nb + trans)
    M = 257
    # both triangles full and different: the kernel must use only its own
    T = rng.standard_normal((nb, nb)) + nb * np.eye(nb)
    X = rng.standard_normal((M, nb))
    out = hp.emu_trsm32(T, X, trans)
    assert hp.trsm_ratio(X, out, T, trans) <= 1.0
    # the first row of the second 256-row block left unsolved
    bad = hp.emu_trsm32(T, X, trans, skip_rows=(256,))
    assert hp.trsm_ratio(X, bad, T, trans) > FAR
    if nb > 1:                             # solved with the other triangle
        assert hp.trsm_ratio(X, hp.emu_trsm32(T, X, 1 - trans), T,
                             trans) > FAR
    T0 =hp.exact_lower(rng, nb) if trans else hp.exact_upper(rng, nb)
    X0 = hp.ints(rng, (M, nb))
    Tm = T0.T if trans else T0
    assert hp.bits_equal(hp.emu_trsm32(T0, X0 @ Tm, trans), X0)


@pytest.mark.parametrize("v", [8, 32, 48, 96, 128])
def test_potrf_tile_emulation(v):
    rng = np.random.default_rng(50 + v)
    A = hp.spd(rng, v)
    F = hp.emu_potrf_tile(A)
    assert hp.potrf_ratio(A, F, width=v) <= 1.0
    L0 = hp.exact_lower(rng, v)
    assert hp.bits_equal(np.tril(hp.emu_potrf_tile(L0 @ L0.T)), L0)
    if v > 32:                             # the solve below block 0 skips a row
        bad = F.copy()
        bad[v - 1, :32] = A[v - 1, :32]
        assert hp.potrf_ratio(A, bad, width=v) > FAR
