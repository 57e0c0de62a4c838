"""Single-GPU solve benchmark: factor once, solve `--reps` times per nrhs,
print the median device ms of the two sweeps, the effective bandwidth
(2 * N^2 * 8 bytes / time: each sweep reads F once) and the normwise
backward error against the host matrix oracle.gen_matrix(N).

    python tools/solve_bench.py [--N 16384] [--v 512] [--nrhs 1,16,128,512]

CONFLUX_SOLVE_SKINNY=0|1 (read once by the library) routes the nrhs <= 16
update through the 128-wide GEMM (0) or the skinny kernel (1);
CONFLUX_SOLVE_BLOCK=<divisor of v> sets the sweep block (default 128 for
larger tiles).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

import conflux_amd  # noqa: E402
from oracle import gen_matrix  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--v", type=int, default=512)
    ap.add_argument("--nrhs", default="1,16,128,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    knob = os.environ.get("CONFLUX_SOLVE_SKINNY", "default")
    rng = np.random.default_rng(0)
    with conflux_amd.Engine(a.N, a.v, 1, 1, 1, rank=-1) as e:
        N = e.Npad
        e.store_factors(True)
        e.init_matrix(42)  # device-side fill == gen_matrix(N), seed 42
        fms = e.factor()
        print(f"N={N} v={a.v} factor {fms:.1f} ms  CONFLUX_SOLVE_SKINNY={knob}")
        A = None if a.no_verify else gen_matrix(N)
        normA = None if A is None else np.linalg.norm(A)
        print(f"{'nrhs':>5} {'ms':>9} {'GB/s':>8} {'eta':>10}")
        for nrhs in (int(x) for x in a.nrhs.split(",")):
            B = rng.standard_normal((N, nrhs))
            e.solve(B)  # warm-up: code objects, allocator
            times = []
            for _ in range(a.reps):
                X, ms = e.solve(B, return_ms=True)
                times.append(ms)
            med = statistics.median(times)
            gbs = 2.0 * N * N * 8 / (med * 1e-3) / 1e9
            eta = float("nan")
            if A is not None:
                eta = np.linalg.norm(B - A @ X) / (
                    normA * np.linalg.norm(X) + np.linalg.norm(B))
            print(f"{nrhs:>5} {med:>9.3f} {gbs:>8.1f} {eta:>10.2e}")
            print(json.dumps(dict(N=N, v=a.v, nrhs=nrhs, skinny=knob,
                                  ms_median=med, ms_all=times, gbs=gbs,
                                  eta=eta)))


if __name__ == "__main__":
    main()
