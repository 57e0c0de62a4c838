"""One rank of the world = 2 guard test of tests/test_dense_gpu.py.

Launched once per rank with tests/shimccl.so preloaded and SHIMCCL_DIR set
(see dist_worker.py): a real (!sim) 1x1x2 engine factors the generator
matrix, then calls every entry point of the device-resident dense interface,
which must refuse (EARG) on every rank before any communication.

usage: dense_dist_worker.py rank out.txt
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))


def main():
    import torch

    import conflux_amd
    from conflux_amd import Engine

    rank, out = int(sys.argv[1]), sys.argv[2]
    N, v = 128, 16
    lib = conflux_amd.lib()
    uid = Engine.make_uid()
    A = torch.eye(N, dtype=torch.float64, device="cuda")
    B = torch.ones((N, 2), dtype=torch.float64, device="cuda")
    perm = torch.zeros((N,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with Engine(N, v, 1, 1, 2, rank=rank, world=2, uid=uid) as e:
        e.store_factors(True)
        e.init_matrix(42)
        e.factor()
        x = ctypes.c_double()
        y = ctypes.c_double()
        codes = [
            lib.conflux_lu_set_matrix_device(e._h, A.data_ptr(), N, N, 0),
            lib.conflux_lu_get_factors_device(e._h, A.data_ptr(), N,
                                              perm.data_ptr()),
            lib.conflux_lu_solve_device(e._h, B.data_ptr(), 2, 2, 0, None),
            lib.conflux_chol_solve_device(e._h, B.data_ptr(), 2, 2, None),
            lib.conflux_lu_slogdet(e._h, ctypes.byref(x), ctypes.byref(y)),
            lib.conflux_chol_logdet(e._h, ctypes.byref(x)),
        ]
        untouched = bool((B == 1.0).all()) and \
            bool((A == torch.eye(N, dtype=torch.float64,
                                 device="cuda")).all())
    with open(out, "w") as f:
        f.write(" ".join(str(c) for c in codes) + f" {int(untouched)}\n")


if __name__ == "__main__":
    main()
