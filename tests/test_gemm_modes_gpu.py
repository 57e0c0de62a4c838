"""launch_dgemm_f64 in every mode it ships, against the longdouble reference
and the derived elementwise bound of tests/_hp_ref.py: all four variants (0, 1
and 3 = k_dgemm_mfma<GemmW4>, <GemmW8>, <GemmBm256>; 2 = k_dgemm_f64_glds), the
capped persistent loop, the strip tile order past its width, the XCD swizzle
at nwg % 8 != 0, the non-temporal epilogue and leading dimensions that differ
from the widths.  Operands sit in canvases of NaN canaries (nothing outside
the M x N window of C may change, no padding may be read into the result), and
every mode also runs an integer case whose result must match bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import _hp_ref as hp

pytestmark = pytest.mark.gpu

SMALL = [(1, 1, 1), (129, 257, 17), (300, 1, 512), (1, 130, 15),
         (128, 128, 16)]
# (385, 1153, 40): 4 x 10 = 40 workgroups (swizzle active), ntn = 10 > 8 with
# a ragged last strip of 2, three K-tiles with a tail of 8.
# (257, 1409, 16): 3 x 12 = 36 workgroups, nwg % 8 == 4.
LARGE = [(385, 1153, 40), (257, 1409, 16)]
SHAPES = SMALL + LARGE
GLDS_SHAPES = [(130, 258, 48), (384, 1154, 32)]
LDS = ["tight", "padded"]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    import conflux_amd
    lib = conflux_amd.lib()
    strip = lib.conflux_lu_debug_set_gemm_strip(8)
    ntc = lib.conflux_lu_debug_set_gemm_ntc(0)
    yield lib
    lib.conflux_lu_debug_set_gemm_strip(strip)
    lib.conflux_lu_debug_set_gemm_ntc(ntc)


_CASES = {}


def case(M, N, K, exact=False):
    """Inputs, longdouble reference and bound: computed once, never written."""
    key = (M, N, K, exact)
    if key not in _CASES:
        rng = np.random.default_rng([M, N, K, int(exact)])
        if exact:
            A, B, C = (hp.ints(rng, s) for s in ((M, K), (K, N), (M, N)))
        else:
            A, B, C = (rng.standard_normal(s) for s in ((M, K), (K, N), (M, N)))
        ref, bound = hp.gemm_ref(A, B, C)
        for x in (A, B, C, ref, bound):
            x.setflags(write=False)
        _CASES[key] = (A, B, C, ref, bound)
    return _CASES[key]


def lds_of(M, N, K, ld, even=False):
    if ld == "tight":
        return K, N, N, M
    if even:
        return K + 4, N + 6, N + 7, M + 3
    return K + 3, N + 5, N + 7, M + 3


def run(lib, variant, maxwg, M, N, K, ld, exact=False, even=False):
    """One launch; returns the M x N window after checking the canaries."""
    A, B, C, _, _ = case(M, N, K, exact)
    lda, ldb, ldc, crows = lds_of(M, N, K, ld, even)
    fA, fB, fC = hp.framed(A, M, lda), hp.framed(B, K, ldb), \
        hp.framed(C, crows, ldc)
    rc = lib.conflux_lu_debug_dgemm_ex(variant, maxwg, M, N, K, lda, ldb, ldc,
                                       crows, _ptr(fA), _ptr(fB), _ptr(fC))
    assert rc == 0
    assert hp.frame_intact(fC, M, N), "wrote outside the M x N window of C"
    return fC[:M, :N].copy()


def ratio(got, M, N, K):
    _, _, _, ref, bound = case(M, N, K)
    r = hp.worst_ratio(np.abs(got.astype(hp.LD) - ref), bound)
    print(f"RATIO gemm {M}x{N}x{K} {r:.3f}")
    return r


def exact_ok(got, M, N, K):
    _, _, _, ref, _ = case(M, N, K, exact=True)
    return hp.bits_equal(got, ref.astype(np.float64))


@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_w8_strip_and_epilogue(lib, M, N, K, ld):
    """Variant 1: strip widths 8 and 1, both epilogues.  The tiles do the same
    arithmetic in every one of them, so all four results are the same bits."""
    outs = []
    try:
        for strip in (8, 1):
            lib.conflux_lu_debug_set_gemm_strip(strip)
            for ntc in (0, 1):
                lib.conflux_lu_debug_set_gemm_ntc(ntc)
                outs.append(run(lib, 1, 0, M, N, K, ld))
                assert exact_ok(run(lib, 1, 0, M, N, K, ld, exact=True),
                                M, N, K), (strip, ntc)
    finally:
        lib.conflux_lu_debug_set_gemm_strip(8)
        lib.conflux_lu_debug_set_gemm_ntc(0)
    assert ratio(outs[0], M, N, K) <= 1.0
    for o in outs[1:]:
        assert hp.bits_equal(o, outs[0])


@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("M,N,K", LARGE)
def test_w8_capped_loop(lib, M, N, K, ld):
    """maxwg > 0 (the look-ahead launch): the persistent loop walks the same
    tiles, so every cap gives the bits of the uncapped launch."""
    nwg = -(-M // 128) * -(-N // 128)
    base = run(lib, 1, 0, M, N, K, ld)
    assert ratio(base, M, N, K) <= 1.0
    for maxwg in (7, 16, nwg, nwg + 5):
        assert hp.bits_equal(run(lib, 1, maxwg, M, N, K, ld), base), maxwg
        assert exact_ok(run(lib, 1, maxwg, M, N, K, ld, exact=True), M, N, K)
    try:                                   # and with the flat tile order
        lib.conflux_lu_debug_set_gemm_strip(1)
        assert hp.bits_equal(run(lib, 1, 7, M, N, K, ld), base)
    finally:
        lib.conflux_lu_debug_set_gemm_strip(8)


@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", [0, 3])
def test_variants_0_and_3(lib, variant, M, N, K, ld):
    assert ratio(run(lib, variant, 0, M, N, K, ld), M, N, K) <= 1.0
    assert exact_ok(run(lib, variant, 0, M, N, K, ld, exact=True), M, N, K)


@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("M,N,K", GLDS_SHAPES)
def test_glds_inside_envelope(lib, M, N, K, ld):
    """Variant 2 where it may run: K % 16 == 0, even lda, ldb and N."""
    got = run(lib, 2, 0, M, N, K, ld, even=True)
    assert ratio(got, M, N, K) <= 1.0
    assert exact_ok(run(lib, 2, 0, M, N, K, ld, exact=True, even=True),
                    M, N, K)


@pytest.mark.parametrize("M,N,K,ld,even", [
    (129, 257, 17, "tight", False),   # K tail, odd N, odd lda and ldb
    (129, 257, 17, "padded", False),
    (130, 258, 48, "padded", False),  # only the leading dimensions are odd
    (128, 128, 8, "tight", True),     # the engine's v = 8: half a K-tile
])
def test_glds_outside_envelope_runs_w8(lib, M, N, K, ld, even):
    """Outside the envelope the launcher must run k_dgemm_mfma<GemmW8>: same
    bits as variant 1, nothing read past the operands (the canaries are
    NaN)."""
    got = run(lib, 2, 0, M, N, K, ld, even=even)
    assert hp.bits_equal(got, run(lib, 1, 0, M, N, K, ld, even=even))
    assert ratio(got, M, N, K) <= 1.0
    assert exact_ok(run(lib, 2, 0, M, N, K, ld, exact=True, even=even),
                    M, N, K)


def test_variant_is_restored(lib):
    """The selected variant holds for one call only: a plain debug_dgemm
    afterwards gives the bits of the default (GemmW8) kernel again."""
    M, N, K = 129, 257, 17
    A, B, C, _, _ = case(M, N, K)
    run(lib, 0, 0, M, N, K, "tight")
    C1 = C.copy()
    assert lib.conflux_lu_debug_dgemm(M, N, K, _ptr(A), _ptr(B), _ptr(C1)) == 0
    if os.environ.get("CONFLUX_GEMM_VARIANT", "1") == "1":
        assert hp.bits_equal(C1, run(lib, 1, 0, M, N, K, "tight"))
    assert ratio(C1, M, N, K) <= 1.0


@pytest.mark.parametrize("bad", [
    dict(variant=4), dict(variant=-1), dict(maxwg=-1), dict(M=0), dict(N=0),
    dict(K=0), dict(lda=15), dict(ldb=31), dict(ldc=31), dict(c_rows=15),
])
def test_bad_arguments_are_refused(lib, bad):
    """EARG before any launch; C comes back untouched."""
    a = dict(variant=1, maxwg=0, M=16, N=32, K=16, lda=16, ldb=32, ldc=32,
             c_rows=16)
    a.update(bad)
    A, B, C = hp.canvas(16, 16), hp.canvas(16, 32), hp.canvas(16, 32)
    rc = lib.conflux_lu_debug_dgemm_ex(
        a["variant"], a["maxwg"], a["M"], a["N"], a["K"], a["lda"], a["ldb"],
        a["ldc"], a["c_rows"], _ptr(A), _ptr(B), _ptr(C))
    assert rc == -1
    assert hp.frame_intact(C, 0, 0)
