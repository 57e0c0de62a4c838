"""Single-GPU solve benchmark: factor once, solve `--reps` times per nrhs,
print the median device ms of the two sweeps, the effective bandwidth
(2 * N^2 * 8 bytes / time: each sweep reads F once) and the normwise
backward error against the host matrix oracle.gen_matrix(N).

    python tools/solve_bench.py [--N 16384] [--v 512] [--nrhs 1,16,128,512]

    python tools/solve_bench.py --refine [--N 16384] [--v 512] [--nrhs 1,16,128]

--refine benchmarks conflux_lu_solve_refined instead: for tournament pivoting
and for the no-pivot fast path it prints the factorization time, the plain
solve, the refined solve (median device ms, passes taken, worst berr before
and after), and — once per nrhs, device-only — the time of one residual
evaluation R = B - A X, of one of its passes over A (a pass handles one
column group) with the effective GB/s over N^2 * 8 B, next to a plain
device-to-device copy of the same N^2 * 8 B in the same run.

    python tools/solve_bench.py --refine --trans [--N 16384] [--v 512]

--refine --trans does the same for conflux_lu_solve_refined_trans (plain
column: conflux_lu_solve_trans), and its residual table times one transposed
pass R = B - A^T X beside one plain pass R = B - A X and the device copy, all
on one buffer in one run, with the ratio of the two passes.

    python tools/solve_bench.py --trans [--rcond] [--N 16384] [--v 512]

--trans benchmarks conflux_lu_solve_trans next to the plain solve: per nrhs
the two alternate within one repetition loop (plain, transposed, plain, ...),
and the medians, the ratio and both backward errors are printed.  --rcond
adds (or, alone, runs only) the condition estimate: conflux_lu_rcond in both
norms `--reps` times — rcond, ||A||, the solves taken, the median device ms
of the estimation loop, and that time over nsolves x the nrhs = 1 plain
solve of the same run.

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


def refine_main(a):
    import ctypes
    lib = conflux_amd.lib()
    rng = np.random.default_rng(0)
    nrhs_list = [int(x) for x in (a.nrhs or "1,16,128").split(",")]
    G = lib.conflux_lu_debug_residual_group_width()
    with conflux_amd.Engine(a.N, a.v, 1, 1, 1, rank=-1) as e:
        plain = e.solve_transposed if a.trans else e.solve
        refined = e.solve_transposed_refined if a.trans else e.solve_refined
        what = "A^T X = B" if a.trans else "A X = B"
        N = e.Npad
        e.store_factors(True)
        e.init_matrix(42)
        Bs = {n: rng.standard_normal((N, n)) for n in nrhs_list}
        for piv in (1, 0):
            e.set_pivoting(piv)
            e.factor()  # warm-up
            fms = e.factor()
            name = "tournament" if piv else "no-pivot"
            print(f"N={N} v={a.v} {name}, {what}: factor {fms:.1f} ms")
            print(f"{'nrhs':>5} {'plain ms':>9} {'refined ms':>10} {'iters':>5} "
                  f"{'berr plain':>11} {'berr refined':>12}")
            for nrhs in nrhs_list:
                B = Bs[nrhs]
                refined(B)  # warm-up: code objects, allocator
                tp, tr = [], []
                for _ in range(a.reps):
                    tp.append(plain(B, return_ms=True)[1])
                    X, info = refined(B, max_iter=a.max_iter,
                                      return_info=True)
                    tr.append(info["ms"])
                b0 = refined(B, max_iter=0,
                             return_info=True)[1]["berr"].max()
                mp, mr = statistics.median(tp), statistics.median(tr)
                print(f"{nrhs:>5} {mp:>9.3f} {mr:>10.3f} {info['iters']:>5} "
                      f"{b0:>11.2e} {info['berr'].max():>12.2e}")
                print(json.dumps(dict(
                    N=N, v=a.v, nrhs=nrhs, pivoting=piv, factor_ms=fms,
                    trans=bool(a.trans),
                    plain_ms_median=mp, refined_ms_median=mr,
                    refined_ms_all=tr, iters=info["iters"], berr_plain=b0,
                    berr_refined=float(info["berr"].max()),
                    ferr=float(info["ferr"].max()))))
    if a.trans:
        return residual_t_table(a, lib, N, nrhs_list, G)
    print(f"residual R = B - A X alone, {N} x {N}, column group {G}:")
    print(f"{'nrhs':>5} {'resid ms':>9} {'passes':>6} {'pass ms':>8} "
          f"{'GB/s':>8} {'copy ms':>8} {'copy GB/s (r+w)':>15}")
    for nrhs in nrhs_list:
        ms_r, ms_c = ctypes.c_double(), ctypes.c_double()
        rc = lib.conflux_lu_debug_residual_dd_bench(
            N, N, nrhs, a.reps, ctypes.byref(ms_r), ctypes.byref(ms_c))
        assert rc == 0, rc
        passes = -(-nrhs // G)
        pass_ms = ms_r.value / passes
        gbs = N * N * 8 / (pass_ms * 1e-3) / 1e9
        cgbs = 2.0 * N * N * 8 / (ms_c.value * 1e-3) / 1e9
        print(f"{nrhs:>5} {ms_r.value:>9.3f} {passes:>6} {pass_ms:>8.3f} "
              f"{gbs:>8.1f} {ms_c.value:>8.3f} {cgbs:>15.1f}")
        print(json.dumps(dict(N=N, nrhs=nrhs, resid_ms=ms_r.value,
                              passes=passes, pass_ms=pass_ms, pass_gbs=gbs,
                              copy_ms=ms_c.value, copy_gbs_rw=cgbs)))


def residual_t_table(a, lib, N, nrhs_list, G):
    import ctypes
    C = lib.conflux_lu_debug_residual_t_chunk()
    print(f"residual alone, {N} x {N}, column group {G}, transposed row "
          f"chunk {C}: R = B - A^T X beside R = B - A X and the device copy")
    print(f"{'nrhs':>5} {'passes':>6} {'T pass ms':>9} {'T GB/s':>8} "
          f"{'pass ms':>8} {'GB/s':>8} {'T/plain':>7} {'copy ms':>8} "
          f"{'copy GB/s (r+w)':>15}")
    for nrhs in nrhs_list:
        runs = []
        for _ in range(a.reps):  # median of reps runs, each the mean of 4
            o = [ctypes.c_double() for _ in range(3)]
            rc = lib.conflux_lu_debug_residual_dd_t_bench(
                N, N, nrhs, 4, *(ctypes.byref(x) for x in o))
            assert rc == 0, rc
            runs.append([x.value for x in o])
        ms_t, ms_r, ms_c = (ctypes.c_double(statistics.median(r[i] for r in runs))
                            for i in range(3))
        passes = -(-nrhs // G)
        pt, pp = ms_t.value / passes, ms_r.value / passes
        gt = N * N * 8 / (pt * 1e-3) / 1e9
        gp = N * N * 8 / (pp * 1e-3) / 1e9
        cgbs = 2.0 * N * N * 8 / (ms_c.value * 1e-3) / 1e9
        print(f"{nrhs:>5} {passes:>6} {pt:>9.3f} {gt:>8.1f} {pp:>8.3f} "
              f"{gp:>8.1f} {pt / pp:>7.2f} {ms_c.value:>8.3f} {cgbs:>15.1f}")
        print(json.dumps(dict(
            N=N, nrhs=nrhs, passes=passes, resid_t_ms=ms_t.value,
            resid_ms=ms_r.value, pass_t_ms=pt, pass_ms=pp, pass_t_gbs=gt,
            pass_gbs=gp, t_over_plain=pt / pp, copy_ms=ms_c.value,
            copy_gbs_rw=cgbs)))


def trans_rcond_main(a):
    rng = np.random.default_rng(0)
    nrhs_list = [int(x) for x in (a.nrhs or "1,16,128").split(",")]
    with conflux_amd.Engine(a.N, a.v, 1, 1, 1, rank=-1) as e:
        N = e.Npad
        e.store_factors(True)
        e.init_matrix(42)  # device-side fill == gen_matrix(N), seed 42
        fms = e.factor()
        print(f"N={N} v={a.v} factor {fms:.1f} ms")
        A = None if a.no_verify else gen_matrix(N)
        normA = None if A is None else np.linalg.norm(A)

        def eta(M, X, B):
            if M is None:
                return float("nan")
            return float(np.linalg.norm(B - M @ X) / (
                normA * np.linalg.norm(X) + np.linalg.norm(B)))

        if a.trans:
            print(f"{'nrhs':>5} {'plain ms':>9} {'trans ms':>9} {'ratio':>6} "
                  f"{'eta plain':>10} {'eta trans':>10}")
            for nrhs in nrhs_list:
                B = rng.standard_normal((N, nrhs))
                e.solve(B)  # warm-up: code objects, allocator
                e.solve_transposed(B)
                tp, tt = [], []
                for _ in range(a.reps):  # alternate within the run
                    X, ms = e.solve(B, return_ms=True)
                    tp.append(ms)
                    Xt, ms = e.solve_transposed(B, return_ms=True)
                    tt.append(ms)
                mp, mt = statistics.median(tp), statistics.median(tt)
                ep = eta(A, X, B)
                et = eta(None if A is None else A.T, Xt, B)
                print(f"{nrhs:>5} {mp:>9.3f} {mt:>9.3f} {mt / mp:>6.2f} "
                      f"{ep:>10.2e} {et:>10.2e}")
                print(json.dumps(dict(
                    N=N, v=a.v, nrhs=nrhs, plain_ms_median=mp,
                    trans_ms_median=mt, plain_ms_all=tp, trans_ms_all=tt,
                    eta_plain=ep, eta_trans=et)))
        if a.rcond:
            b1 = rng.standard_normal(N)
            e.solve(b1)
            t1 = statistics.median(
                e.solve(b1, return_ms=True)[1] for _ in range(a.reps))
            print(f"{'norm':>5} {'rcond':>11} {'anorm':>11} {'nsolves':>7} "
                  f"{'ms':>9} {'ms/(nsolves*solve)':>18}   "
                  f"(nrhs=1 solve {t1:.3f} ms)")
            for which in ("1", "I"):
                e.rcond(which)  # warm-up; also caches ||A||
                ts = []
                for _ in range(a.reps):
                    rc, info = e.rcond(which, return_info=True)
                    ts.append(info["ms"])
                med = statistics.median(ts)
                over = med / (info["nsolves"] * t1)
                print(f"{which:>5} {rc:>11.4e} {info['anorm']:>11.4e} "
                      f"{info['nsolves']:>7} {med:>9.3f} {over:>18.2f}")
                print(json.dumps(dict(
                    N=N, v=a.v, norm=which, rcond=rc, anorm=info["anorm"],
                    nsolves=info["nsolves"], ms_median=med, ms_all=ts,
                    solve1_ms=t1, over_nsolves_x_solve=over)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--v", type=int, default=512)
    ap.add_argument("--nrhs", default=None,
                    help="default 1,16,128,512 (--refine, --trans: 1,16,128)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--refine", action="store_true",
                    help="benchmark the refined solve and its residual")
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--trans", action="store_true",
                    help="benchmark the transposed solve next to the plain")
    ap.add_argument("--rcond", action="store_true",
                    help="benchmark the condition estimate")
    a = ap.parse_args()
    if a.refine:
        return refine_main(a)
    if a.trans or a.rcond:
        return trans_rcond_main(a)
    a.nrhs = a.nrhs or "1,16,128,512"
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
