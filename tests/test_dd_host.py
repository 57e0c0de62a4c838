"""Host test of the compensated dot product (conflux_amd/csrc/dd.hpp): a
stand-alone program built with hipcc's host clang++ (no GPU code) against
exact rational arithmetic.

Bar (the Dot2 bound of Ogita, Rump and Oishi, with slack 2):
    |got - exact| <= 2 u |exact| + 2 (K+1)^2 u^2 sum|a_k x_k|,   u = 2^-53.
The cancelling cases have exact ~ u sum|a_k x_k|, where a plain fp64 dot has
no correct digit; the test asserts that the plain dot misses the bar there,
so passing it means something.

Where the CPU has FMA the program is built with -mfma -ffp-contract=fast,
the contraction mode the device compiler uses: the header has to defend its
error-free transformations against it by itself.
"""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "conflux_amd", "csrc")
U = Fraction(1, 2 ** 53)


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


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma " in line + " "
    except OSError:
        pass
    return False


def _cancelling(rng, K):
    """First half random, second half its negation perturbed in the last few
    bits: the exact dot is a few u * sum|a x|."""
    m = K // 2
    a = rng.standard_normal(m)
    x = rng.standard_normal(m)
    d = rng.integers(1, 5, m) * 2.0 ** -52
    aa = np.concatenate([a, a])
    xx = np.concatenate([x, -x * (1.0 + d)])
    if K % 2:
        aa = np.append(aa, rng.standard_normal() * 2.0 ** -55)
        xx = np.append(xx, rng.standard_normal())
    p = rng.permutation(K)
    return aa[p], xx[p]


def _cases():
    rng = np.random.default_rng(2024)
    out = []
    for K in (1, 2, 63, 1000):
        out.append(("random", rng.standard_normal(K), rng.standard_normal(K)))
        if K > 1:
            out.append(("cancel",) + _cancelling(rng, K))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("dd_host")
    exe = str(d / "dd_host_main")
    cmd = [_host_clangxx(), "-O2", "-std=c++17", "-I", CSRC,
           os.path.join(HERE, "dd_host_main.cpp"), "-o", exe]
    if _cpu_has_fma():
        cmd[1:1] = ["-mfma", "-ffp-contract=fast"]
    subprocess.run(cmd, check=True)
    cases = _cases()
    inp = d / "cases.txt"
    with open(inp, "w") as f:
        f.write(f"{len(cases)}\n")
        for _, a, x in cases:
            f.write(f"{len(a)}\n")
            for ak, xk in zip(a, x):
                f.write(f"{float(ak).hex()} {float(xk).hex()}\n")
    out = subprocess.run([exe, str(inp)], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    got = [tuple(float.fromhex(t) for t in line.split())
           for line in out if line.strip()]
    assert len(got) == len(cases)
    return cases, got


def _bar(a, x):
    exact = sum(Fraction(float(ak)) * Fraction(float(xk))
                for ak, xk in zip(a, x))
    sabs = sum(abs(Fraction(float(ak)) * Fraction(float(xk)))
               for ak, xk in zip(a, x))
    K = len(a)
    return exact, 2 * U * abs(exact) + 2 * (K + 1) ** 2 * U * U * sabs


def test_dot2_meets_the_bound(results):
    cases, got = results
    for (kind, a, x), (one, merged) in zip(cases, got):
        exact, bar = _bar(a, x)
        for name, g in (("one accumulator", one), ("merged", merged)):
            err = abs(Fraction(g) - exact)
            print(f"{kind} K={len(a)} {name}: err={float(err):.3g} "
                  f"bar={float(bar):.3g} exact={float(exact):.3g}")
            assert err <= bar, (kind, len(a), name, float(err), float(bar))


def test_plain_dot_misses_the_bound_where_it_cancels(results):
    cases, _ = results
    seen = 0
    for kind, a, x in cases:
        if kind != "cancel":
            continue
        exact, bar = _bar(a, x)
        plain = 0.0
        for ak, xk in zip(a, x):
            plain += float(ak) * float(xk)
        err = abs(Fraction(plain) - exact)
        print(f"cancel K={len(a)} plain fp64: err={float(err):.3g} "
              f"bar={float(bar):.3g}")
        assert err > bar, (len(a), float(err), float(bar))
        seen += 1
    assert seen == 3
