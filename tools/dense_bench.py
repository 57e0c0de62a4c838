"""Single-GPU benchmark of the device-resident dense interface
(conflux_lu_set_matrix_device / get_factors_device / solve_device).

    python tools/dense_bench.py [--N 16384] [--v 512] [--nrhs 1,16,128]

Four tables, each figure the median of `--reps` wall-clock times around a
call that returns with the engine's stream synchronized:

  import/export  the row-major import, the column-major import and the
                 export of the N x N matrix, each next to a plain device copy
                 of the same N^2 * 8 bytes (torch copy_ + synchronize) taken
                 inside the same repetition loop; GB/s counts the bytes read
                 plus the bytes written.
  solve          solve_device (B and X stay on the device) against the host
                 solve (B up and X down over PCIe) per nrhs: wall ms of the
                 whole call and the device ms of the two sweeps.
  refined        solve_refined_device against the host refined solve on
                 no-pivot factors, A X = B and A^T X = B, per nrhs: wall ms of
                 the whole call and the device ms of the refinement loop.
  end to end     a device tensor A and B to a device tensor X:
                 device path = set_matrix_device + factor + solve_device;
                 host path   = A and B to the host, set_matrix_local (on one
                 rank the engine's layout is plain row-major), factor, solve,
                 X back to the device.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import conflux_amd  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--v", type=int, default=512)
    ap.add_argument("--nrhs", default="1,16,128")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, v = a.N, a.v
    nrhs_list = [int(x) for x in a.nrhs.split(",")]
    med = statistics.median
    gen = torch.Generator(device="cuda").manual_seed(0)
    # well conditioned without being dominant: U[0,1) + sqrt(N) on the diagonal
    A = torch.rand((N, N), dtype=torch.float64, device="cuda", generator=gen)
    A += (N ** 0.5) * torch.eye(N, dtype=torch.float64, device="cuda")
    At = A.T.contiguous()  # the column-major image of A
    scratch = torch.empty_like(A)
    nbytes = 2.0 * N * N * 8  # read + write

    with conflux_amd.Engine(N, v, 1, 1, 1, rank=0, world=1) as e:
        assert e.Npad == N, "pick N a multiple of v"
        e.store_factors(True)
        pA, pAt, pS = A.data_ptr(), At.data_ptr(), scratch.data_ptr()
        e.set_matrix_device(pA, N, N, 0)  # warm-up: code objects
        e.set_matrix_device(pAt, N, N, 1)
        fms = e.factor()
        e.get_factors_device(pS, N, None)
        scratch.copy_(A)
        steps = [
            ("import row-major", lambda: e.set_matrix_device(pA, N, N, 0)),
            ("import col-major", lambda: e.set_matrix_device(pAt, N, N, 1)),
            ("export", lambda: e.get_factors_device(pS, N, None)),
        ]
        print(f"N={N} v={v} factor {fms:.1f} ms")
        print(f"{'step':>17} {'ms':>8} {'GB/s':>8} {'copy ms':>8} "
              f"{'copy GB/s':>9} {'vs copy':>7}")
        for name, fn in steps:
            ts, cs = [], []
            for _ in range(a.reps):  # alternate within the run
                ts.append(wall_ms(fn))
                cs.append(wall_ms(lambda: scratch.copy_(A)))
            m, c = med(ts), med(cs)
            print(f"{name:>17} {m:>8.3f} {nbytes / m / 1e6:>8.1f} {c:>8.3f} "
                  f"{nbytes / c / 1e6:>9.1f} {c / m:>7.2f}")
            print(json.dumps(dict(N=N, v=v, step=name, ms_median=m, ms_all=ts,
                                  gbs=nbytes / m / 1e6, copy_ms_median=c,
                                  copy_ms_all=cs, copy_gbs=nbytes / c / 1e6)))

        e.set_matrix_device(pA, N, N, 0)
        e.factor()
        print(f"{'nrhs':>5} {'dev wall':>9} {'dev sweeps':>10} {'host wall':>9} "
              f"{'host sweeps':>11} {'wall ratio':>10}")
        for nrhs in nrhs_list:
            B = torch.randn((N, nrhs), dtype=torch.float64, device="cuda",
                            generator=gen)
            Bh = B.cpu().numpy()
            X = B.clone()
            e.solve_device(X.data_ptr(), nrhs, nrhs)  # warm-up
            e.solve(Bh)
            td, sd, th, sh = [], [], [], []
            for _ in range(a.reps):
                X.copy_(B)
                box = []
                td.append(wall_ms(lambda: box.append(
                    e.solve_device(X.data_ptr(), nrhs, nrhs))))
                sd.append(box[0])
                box = []
                th.append(wall_ms(lambda: box.append(
                    e.solve(Bh, return_ms=True)[1])))
                sh.append(box[0])
            same = bool(np.array_equal(X.cpu().numpy(), e.solve(Bh)))
            print(f"{nrhs:>5} {med(td):>9.3f} {med(sd):>10.3f} "
                  f"{med(th):>9.3f} {med(sh):>11.3f} "
                  f"{med(th) / med(td):>10.2f}")
            print(json.dumps(dict(
                N=N, v=v, nrhs=nrhs, dev_wall_ms=med(td), dev_sweeps_ms=med(sd),
                host_wall_ms=med(th), host_sweeps_ms=med(sh),
                dev_wall_all=td, host_wall_all=th, bitwise_equal=same)))

        # refined solves: no-pivot factors, plain and transposed
        e.set_pivoting(0)
        e.set_matrix_device(pA, N, N, 0)
        e.factor()
        print(f"{'refined':>9} {'nrhs':>5} {'dev wall':>9} {'dev loop':>9} "
              f"{'host wall':>9} {'host loop':>9} {'wall ratio':>10} "
              f"{'iters':>5} {'berr':>9}")
        for trans in (False, True):
            hostfn = e.solve_transposed_refined if trans else e.solve_refined
            name = "A^T X = B" if trans else "A X = B"
            for nrhs in nrhs_list:
                B = torch.randn((N, nrhs), dtype=torch.float64, device="cuda",
                                generator=gen)
                Bh = B.cpu().numpy()
                X = B.clone()
                e.solve_refined_device(X.data_ptr(), nrhs, nrhs, trans=trans)
                hostfn(Bh)  # warm-up
                td, sd, th, sh = [], [], [], []
                for _ in range(a.reps):
                    X.copy_(B)
                    box = []
                    td.append(wall_ms(lambda: box.append(
                        e.solve_refined_device(X.data_ptr(), nrhs, nrhs,
                                               trans=trans))))
                    info = box[0]
                    sd.append(info["ms"])
                    box = []
                    th.append(wall_ms(lambda: box.append(
                        hostfn(Bh, return_info=True))))
                    sh.append(box[0][1]["ms"])
                same = bool(np.array_equal(X.cpu().numpy(), box[0][0]))
                print(f"{name:>9} {nrhs:>5} {med(td):>9.3f} {med(sd):>9.3f} "
                      f"{med(th):>9.3f} {med(sh):>9.3f} "
                      f"{med(th) / med(td):>10.2f} {info['iters']:>5} "
                      f"{info['berr'].max():>9.2e}")
                print(json.dumps(dict(
                    N=N, v=v, nrhs=nrhs, refined=True, trans=trans,
                    dev_wall_ms=med(td), dev_loop_ms=med(sd),
                    host_wall_ms=med(th), host_loop_ms=med(sh),
                    dev_wall_all=td, host_wall_all=th, iters=info["iters"],
                    berr=float(info["berr"].max()), bitwise_equal=same)))
        e.set_pivoting(1)

        nrhs = nrhs_list[-1]
        B = torch.randn((N, nrhs), dtype=torch.float64, device="cuda",
                        generator=gen)

        def dev_path():
            X = B.clone()
            e.set_matrix_device(pA, N, N, 0)
            e.factor()
            e.solve_device(X.data_ptr(), nrhs, nrhs)
            return X

        def host_path():
            e.set_matrix_local(A.cpu().numpy())
            e.factor()
            return torch.from_numpy(e.solve(B.cpu().numpy())).cuda()

        dev_path()
        host_path()
        td, th = [], []
        for _ in range(a.reps):
            td.append(wall_ms(dev_path))
            th.append(wall_ms(host_path))
        print(f"end to end, nrhs={nrhs}: device path {med(td):.1f} ms, "
              f"host path {med(th):.1f} ms")
        print(json.dumps(dict(N=N, v=v, nrhs=nrhs, e2e_dev_ms=med(td),
                              e2e_host_ms=med(th), e2e_dev_all=td,
                              e2e_host_all=th)))


if __name__ == "__main__":
    main()
