"""GPU tests of the one-rank direct step (CONFLUX_ONE_RANK_DIRECT).

On the one-rank grid (one process, Px = Py = Pz = 1, not the simulation) the
stretch between two panel chains drops the staging that only mirrors the
distributed exchanges: the panel solves read A11 and write the GEMM operands
directly (bit 1), the row push of A11 is sliced (bit 2) and the column block
of the panel just factored is neither solved for nor updated (bit 4).  Mode 0
(conflux_lu_debug_set_one_rank_direct(0)) keeps the staged path.  No bit
changes or reorders a floating-point operation on an element that is read
afterwards, so every comparison between modes here is np.array_equal, never
a tolerance; the oracle comparison uses the bounds of tests/test_engine_gpu.py
(pivots exact, factors within 1e-11).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import Params, gen_matrix, lu_oracle  # noqa: E402

ALL = 7


@pytest.fixture(scope="module")
def eng():
    import conflux_amd
    return conflux_amd


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------- the switch -------------------------------------------------

def test_switch_returns_previous_mode(eng):
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_one_rank_direct(0)
    try:
        assert 0 <= prev <= ALL
        assert lib.conflux_lu_debug_set_one_rank_direct(ALL) == 0
        assert lib.conflux_lu_debug_set_one_rank_direct(2) == ALL
        assert lib.conflux_lu_debug_set_one_rank_direct(5) == 2
        assert lib.conflux_lu_debug_set_one_rank_direct(0) == 5
    finally:
        lib.conflux_lu_debug_set_one_rank_direct(prev)


# ---------------- stripe solves: out of place against in place ---------------

def upper_tri(rng, v):
    U = np.triu(rng.uniform(-1, 1, (v, v)), 1) * (0.5 / v)
    d = rng.uniform(1, 2, v) * rng.choice([-1.0, 1.0], v)
    return U + np.diag(d)


def unit_lower_tri(rng, v):
    return np.tril(rng.uniform(-1, 1, (v, v)), -1) * (0.5 / v) + np.eye(v)


def solve_in_place_old(eng, side_right, v, n, T, W):
    """The window alone (tight leading dimension) through the old in-place
    launch signature: the bitwise reference."""
    X = np.ascontiguousarray(W).copy()
    rc = eng.lib().conflux_lu_debug_trsm_ld(
        side_right, 0, v, n, X.shape[1], 0, _p(np.ascontiguousarray(T)), _p(X))
    assert rc == 0
    return X


def solve_oop(eng, side_right, v, n, T, Xs, soff, Xd, doff):
    """Returns (Xs after, Xd after); Xd None = in place in Xs through the new
    signature."""
    S = np.ascontiguousarray(Xs).copy()
    D = None if Xd is None else np.ascontiguousarray(Xd).copy()
    rc = eng.lib().conflux_lu_debug_trsm_oop(
        side_right, v, n, S.shape[1], soff, 0 if D is None else D.shape[1],
        doff, _p(np.ascontiguousarray(T)), _p(S), None if D is None else _p(D))
    assert rc == 0
    return S, D


def check_oop(eng, side_right, v, n, T, rng, lds, soff, ldd, doff, tag):
    rows = n if side_right else v
    w = v if side_right else n
    Xs = rng.standard_normal((rows, lds))
    Xd = rng.standard_normal((rows, ldd))  # must be overwritten in the window
    ref = solve_in_place_old(eng, side_right, v, n, T, Xs[:, soff:soff + w])
    S, D = solve_oop(eng, side_right, v, n, T, Xs, soff, Xd, doff)
    ndiff = int(np.count_nonzero(D[:, doff:doff + w] != ref))
    print(f"{tag} lds={lds} soff={soff} ldd={ldd} doff={doff}: "
          f"differ={ndiff}")
    assert np.isfinite(D).all(), tag
    assert np.array_equal(D[:, doff:doff + w], ref), tag
    assert np.array_equal(S, Xs), f"{tag}: source written"
    keep = np.ones(ldd, bool)
    keep[doff:doff + w] = False
    assert np.array_equal(D[:, keep], Xd[:, keep]), f"{tag}: outside window"
    # in place through the new signature
    S2, _ = solve_oop(eng, side_right, v, n, T, Xs, soff, None, 0)
    assert np.array_equal(S2[:, soff:soff + w], ref), f"{tag}: in place"
    keep = np.ones(lds, bool)
    keep[soff:soff + w] = False
    assert np.array_equal(S2[:, keep], Xs[:, keep]), f"{tag}: in place window"
    return ref


SIZES = [1, 31, 33, 100]  # a single row / column, ragged stripes, > 3 blocks


@pytest.mark.parametrize("v", [64, 512])
def test_right_solve_out_of_place_bitwise(eng, v):
    """M x v window of a wider source (a 100 x 64 block inside a 100 x 200
    array at v = 64) into a destination of another leading dimension: wider
    with an offset, and tight as the engine's A10Rcv."""
    rng = np.random.default_rng(300 + v)
    U = upper_tri(rng, v)
    for M in SIZES:
        for (lds, soff, ldd, doff) in [(v + 136, 72, v + 8, 3),
                                       (v + 136, 72, v, 0)]:
            ref = check_oop(eng, 1, v, M, U, rng, lds, soff, ldd, doff,
                            f"right v={v} M={M}")
        assert ref.shape == (M, v)


@pytest.mark.parametrize("v", [64, 512])
def test_left_solve_out_of_place_bitwise(eng, v):
    """v x N window of a wider source (the pivot rows in A11) into a
    destination of another leading dimension."""
    rng = np.random.default_rng(400 + v)
    L = unit_lower_tri(rng, v)
    for N in SIZES:
        for (lds, soff, ldd, doff) in [(N + 100, 37, N + 5, 2),
                                       (N + 100, 37, N + 64, 64)]:
            ref = check_oop(eng, 0, v, N, L, rng, lds, soff, ldd, doff,
                            f"left v={v} N={N}")
        assert ref.shape == (v, N)


# ---------------- whole factorizations: mode 0 against the others ------------

def matrix(kind, n):
    """n x n: seeded random; pivots already on the diagonal (no row moves:
    the early and late lists are empty); pivots from the far end (dominant
    anti-diagonal: every pivot outside the window, the lists are full)."""
    A = gen_matrix(n)
    if kind == "random":
        return A
    D = A / np.abs(A).max() + 2.0 * n * np.eye(n)
    return D if kind == "diag" else np.ascontiguousarray(D[::-1])


def factor_one_rank(eng, mode, N, v, kind, store=True):
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_one_rank_direct(mode)
    try:
        with eng.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
            A = np.eye(e.Npad)  # padded by create: identity outside N x N
            A[:N, :N] = matrix(kind, N)
            e.store_factors(store)
            e.set_matrix_local(A)
            e.factor()
            return e.get_perm(), (e.get_F_local() if store else None)
    finally:
        lib.conflux_lu_debug_set_one_rank_direct(prev)


_ref = {}


def reference(eng, N, v, kind, store=True):
    """Mode 0, computed once per case and shared."""
    key = (N, v, kind, store)
    if key not in _ref:
        _ref[key] = factor_one_rank(eng, 0, N, v, kind, store)
        for a in _ref[key]:
            if a is not None:
                a.setflags(write=False)
    return _ref[key]


def assert_same(r0, r1, tag):
    (p0, F0), (p1, F1) = r0, r1
    if F0 is not None:
        print(f"{tag}: factor elements that differ = "
              f"{np.count_nonzero(F0 != F1)}")
        assert np.isfinite(F1).all(), tag
    print(f"{tag}: pivots that differ = {np.count_nonzero(p0 != p1)}")
    assert np.array_equal(p0, p1), f"{tag}: perm"
    if F0 is not None:
        assert np.array_equal(F0, F1), f"{tag}: factors"


# (256, 64): four steps, the smallest with a look-ahead step, a slice and a
# non-empty rest; (1024, 128): eight steps; (1536, 512): the bench's tile;
# (1000, 128): padded by create
@pytest.mark.parametrize("kind", ["random", "diag", "antidiag"])
@pytest.mark.parametrize("N,v", [(256, 64), (1024, 128), (1536, 512),
                                 (1000, 128)])
def test_factorization_bitwise_default_mode(eng, N, v, kind):
    r0 = reference(eng, N, v, kind)
    r1 = factor_one_rank(eng, ALL, N, v, kind)
    assert_same(r0, r1, f"N={N} v={v} {kind} mode {ALL}")
    npad = len(r1[0])
    if kind == "diag":  # the case is what it claims: no row moved
        assert np.array_equal(r1[0], np.arange(npad))
    if kind == "antidiag":  # every pivot row came from the far end
        assert np.array_equal(r1[0][:N], np.arange(N)[::-1])
        assert np.array_equal(r1[0][N:], np.arange(N, npad))


def test_process_default_is_all_bits(eng):
    """What an engine runs without the setter: every bit, unless the
    environment says otherwise."""
    import os
    lib = eng.lib()
    prev = lib.conflux_lu_debug_set_one_rank_direct(0)
    lib.conflux_lu_debug_set_one_rank_direct(prev)
    if "CONFLUX_ONE_RANK_DIRECT" not in os.environ:
        assert prev == ALL


@pytest.mark.parametrize("bit", [1, 2, 4])
def test_each_bit_alone_bitwise(eng, bit):
    N, v = 1024, 128
    r0 = reference(eng, N, v, "random")
    r1 = factor_one_rank(eng, bit, N, v, "random")
    assert_same(r0, r1, f"N={N} v={v} random mode {bit}")


def test_perm_only_without_stored_factors(eng):
    """store_factors off, the benchmark's setting: the permutation alone."""
    N, v = 1024, 128
    r0 = reference(eng, N, v, "random", store=False)
    r1 = factor_one_rank(eng, ALL, N, v, "random", store=False)
    assert_same(r0, r1, f"N={N} v={v} random, factors not stored")
    assert np.array_equal(r1[0], reference(eng, N, v, "random")[0])


def test_sequential_mode_bitwise(eng, monkeypatch):
    """CONFLUX_LOOKAHEAD=0 (read per step): no slice, one full push, the
    direct solves and the dead block still apply."""
    N, v = 1024, 128
    r0 = reference(eng, N, v, "random")
    monkeypatch.setenv("CONFLUX_LOOKAHEAD", "0")
    r1 = factor_one_rank(eng, ALL, N, v, "random")
    assert_same(r0, r1, f"N={N} v={v} random mode {ALL}, sequential")
    r2 = factor_one_rank(eng, 0, N, v, "random")
    assert_same(r0, r2, f"N={N} v={v} random mode 0, sequential")


_GUARD_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import conflux_amd
from test_one_rank_direct_gpu import ALL, factor_one_rank
out = {}
for mode in (ALL, 0):
    perm, F = factor_one_rank(conflux_amd, mode, 1024, 128, "random")
    out["perm%d" % mode], out["F%d" % mode] = perm, F
np.savez(sys.argv[3], **out)
"""


def test_residency_guard_bitwise(eng, tmp_path):
    """The look-ahead's residency guard: with CONFLUX_GEMM_CAP=510 (read once
    per process, hence the fresh child) the capped update leaves one CU free.
    At N = 1024, v = 128 the next panel has 896, 768, 640, 512, ... rows: 4,
    3, 3 blocks of 256 rows at two per CU need two CUs, so the guard turns
    the look-ahead off at steps 0 to 2 while the slice-first solve stays on;
    from step 3 on the panel fits and runs concurrently under the cap.  Same
    pivots and factors as this process's default-cap runs, in both modes."""
    import os
    import subprocess
    import sys
    N, v = 1024, 128
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "guard.npz")
    env = dict(os.environ, CONFLUX_GEMM_CAP="510")
    subprocess.run([sys.executable, "-c", _GUARD_CHILD,
                    os.path.join(here, ".."), here, out],
                   env=env, check=True, timeout=120)
    got = np.load(out)
    r0 = reference(eng, N, v, "random")
    r7 = factor_one_rank(eng, ALL, N, v, "random")
    for mode, mine in ((ALL, r7), (0, r0)):
        child = (got[f"perm{mode}"], got[f"F{mode}"])
        assert_same(mine, child, f"N={N} v={v} cap 510 mode {mode}")
        assert_same(r0, child, f"N={N} v={v} cap 510 mode {mode} vs mode 0")


def test_against_oracle(eng):
    N, v = 1024, 128
    A = matrix("random", N)
    perm, F = factor_one_rank(eng, ALL, N, v, "random")
    ref = lu_oracle(A, Params(N, v, 1, 1, 1))
    err = np.abs(F - ref["F"]).max()
    print(f"oracle: pivots that differ = "
          f"{np.count_nonzero(perm != ref['perm'])}, max |F - F_ref| = "
          f"{err:.3e}")
    assert np.array_equal(perm, ref["perm"])
    assert err < 1e-11
