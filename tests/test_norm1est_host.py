"""Host test of the 1-norm estimator (conflux_amd/csrc/norm1est.hpp): a
stand-alone program built with hipcc's host clang++ (no GPU code) factors
each matrix with its own partial-pivot elimination and runs the estimator
with host callbacks, in both norms.

Bars, rcond_est = 1 / (||A|| est||A^-1||) against the exact
rcond_true = 1 / (||A|| ||A^-1||) from numpy.linalg.inv:
    1 - 1e-3 <= rcond_est / rcond_true <= 3.
The estimator is a lower bound on ||A^-1||, so the ratio is >= 1 up to the
rounding of the solves (1e-3 covers cond 1e10 at n = 256); the factor 3 is
the usual quality of Higham's estimator, a condition and not a guarantee —
LAPACK's dgecon on exactly these inputs gives the same ratios as this
header, between 1.000 and 2.69 (the largest on normal96 in the inf-norm;
all others are below 1.62).

Against scipy's dgecon, on the inputs with cond <= 1e7, the estimate itself
agrees to relative 1e-6: that pins the iteration (start vector, sign
vector, first-max argmax, stopping rules, safeguard), not just its quality.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import gen_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "conflux_amd", "csrc")
SIZES = (64, 96, 256)


def _host_clangxx():
    cands = []
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root:
            cands.append(os.path.join(root, "lib", "llvm", "bin", "clang++"))
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.join(os.path.dirname(os.path.realpath(hipcc)),
                                  "..", "lib", "llvm", "bin", "clang++"))
    for c in cands:
        if os.path.exists(c):
            return c
    raise AssertionError(f"hipcc's host clang++ not found (tried {cands})")


def _prescribed(rng, n, lo):
    """Singular values logspace(0, lo) between random orthogonal factors."""
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q1 * np.logspace(0, lo, n)) @ Q2.T


def _cases():
    """(name, A, compare with dgecon)"""
    out = []
    for n in SIZES:
        rng = np.random.default_rng(7000 + n)
        out.append((f"gen{n}", gen_matrix(n), True))
        out.append((f"normal{n}", rng.standard_normal((n, n)), True))
        out.append((f"diagdom{n}", rng.random((n, n)) + n * np.eye(n), True))
        out.append((f"sv1e-6_{n}", _prescribed(rng, n, -6), True))
        out.append((f"sv1e-10_{n}", _prescribed(rng, n, -10), False))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("norm1est_host")
    exe = str(d / "norm1est_host_main")
    subprocess.run([_host_clangxx(), "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(HERE, "norm1est_host_main.cpp"), "-o", exe],
                   check=True)
    cases = _cases()
    inp = d / "cases.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _, A, _ in cases:
            f.write(struct.pack("<i", A.shape[0]))
            f.write(np.ascontiguousarray(A, dtype="<f8").tobytes())
    lines = [ln for ln in subprocess.run(
        [exe, str(inp)], check=True, capture_output=True,
        text=True).stdout.split("\n") if ln.strip()]
    assert len(lines) == len(cases) + 1
    got = []
    for ln in lines[:-1]:
        e1, n1, ei, ni = ln.split()
        got.append({"1": (float.fromhex(e1), int(n1)),
                    "I": (float.fromhex(ei), int(ni))})
    last = lines[-1].split()
    return cases, got, (float.fromhex(last[0]), int(last[1]))


def _norm(M, which):
    return np.linalg.norm(M, 1 if which == "1" else np.inf)


def test_estimate_against_the_exact_condition_number(results):
    cases, got, _ = results
    for (name, A, _), g in zip(cases, got):
        Ainv = np.linalg.inv(A)
        for which in ("1", "I"):
            est, ns = g[which]
            anorm = _norm(A, which)
            rc_est = 1.0 / (anorm * est)
            rc_true = 1.0 / (anorm * _norm(Ainv, which))
            ratio = rc_est / rc_true
            print(f"{name} norm={which}: rcond_est={rc_est:.6g} "
                  f"rcond_true={rc_true:.6g} ratio={ratio:.6f} nsolves={ns}")
            assert 1 - 1e-3 <= ratio <= 3, (name, which, ratio)
            assert 1 <= ns <= 12, (name, which, ns)


def test_estimate_agrees_with_dgecon(results):
    from scipy.linalg import lapack
    cases, got, _ = results
    seen = 0
    for (name, A, cmp), g in zip(cases, got):
        if not cmp:
            continue
        lu, _, info = lapack.dgetrf(A)
        assert info == 0
        for which in ("1", "I"):
            anorm = _norm(A, which)
            rc, info = lapack.dgecon(lu, anorm, norm=which)
            assert info == 0
            ref = 1.0 / (rc * anorm)
            est = g[which][0]
            rel = abs(est - ref) / ref
            print(f"{name} norm={which}: est={est:.10g} dgecon={ref:.10g} "
                  f"rel={rel:.3g}")
            assert rel <= 1e-6, (name, which, est, ref)
            seen += 1
    assert seen == 2 * 4 * len(SIZES)


def test_non_finite_estimate_gives_rcond_zero(results):
    _, _, (rcond, ns) = results
    assert rcond == 0.0
    assert 1 <= ns <= 12
