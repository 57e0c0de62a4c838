"""One rank of the world = 2 guard test of tests/test_trans_rcond_gpu.py.

Launched once per rank with tests/shimccl.so preloaded and SHIMCCL_DIR set
(see dist_worker.py): a real (!sim) 1x1x2 engine factors the generator
matrix, then calls the transposed solve and the two condition estimates,
which must refuse (EARG) on every rank before any communication.

usage: trans_rcond_dist_worker.py rank out.txt
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))


def main():
    import numpy as np

    import conflux_amd
    from conflux_amd import Engine

    rank, out = int(sys.argv[1]), sys.argv[2]
    N, v = 128, 16
    lib = conflux_amd.lib()
    uid = Engine.make_uid()
    with Engine(N, v, 1, 1, 2, rank=rank, world=2, uid=uid) as e:
        e.store_factors(True)
        e.init_matrix(42)
        e.factor()
        B = np.ones((N, 2))
        rc = ctypes.c_double()
        codes = [
            lib.conflux_lu_solve_trans(
                e._h, B.ctypes.data_as(ctypes.c_void_p), 2, None),
            lib.conflux_lu_rcond(e._h, 0, ctypes.byref(rc), None, None, None),
            lib.conflux_lu_rcond(e._h, 1, ctypes.byref(rc), None, None, None),
            lib.conflux_chol_rcond(e._h, ctypes.byref(rc), None, None, None),
        ]
        untouched = bool((B == 1.0).all())
    with open(out, "w") as f:
        f.write(" ".join(str(c) for c in codes) + f" {int(untouched)}\n")


if __name__ == "__main__":
    main()
