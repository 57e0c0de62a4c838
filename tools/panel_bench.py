import sys, os, ctypes, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, conflux_amd
lib = conflux_amd.lib()
# The leaf kernel and its hand-off form come from the environment, so one
# script times every combination stand-alone:
#   CONFLUX_PANEL_REG=0|1      k_panel_factor | register-resident leaf
#   CONFLUX_PANEL_PUBLISH=0|1  sc1 payload + drain + key | granule payload
#   CONFLUX_PANEL_PHASE_STATS=1 adds the per-phase cycle totals
reg = lib.conflux_lu_debug_set_panel_reg(0)
lib.conflux_lu_debug_set_panel_reg(reg)
pub = lib.conflux_lu_debug_set_panel_publish(0)
lib.conflux_lu_debug_set_panel_publish(pub)
stats = lib.conflux_lu_debug_set_panel_phase_stats(0)
lib.conflux_lu_debug_set_panel_phase_stats(stats)
print(f"CONFLUX_PANEL_REG={reg} CONFLUX_PANEL_PUBLISH={pub} "
      f"CONFLUX_PANEL_PHASE_STATS={stats}")
rng = np.random.default_rng(5)
# warmup: first kernel launch in a fresh process pays code-object load
_P = np.ascontiguousarray(5 + rng.random((1024, 512)))
_ip = np.zeros(512, dtype=np.int32)
lib.conflux_lu_debug_getrf(1024, 512, _P.ctypes.data_as(ctypes.c_void_p),
                           _ip.ctypes.data_as(ctypes.c_void_p))
for (n, v) in [(16384, 512), (32768, 512), (1024, 512)]:
    P = np.ascontiguousarray(5 + rng.random((n, v)))
    ipiv = np.zeros(v, dtype=np.int32)
    t0 = time.perf_counter()
    rc = lib.conflux_lu_debug_getrf(n, v, P.ctypes.data_as(ctypes.c_void_p), ipiv.ctypes.data_as(ctypes.c_void_p))
    dt = time.perf_counter() - t0
    print(f"getrf n={n} v={v}: {dt*1e3:.1f} ms ({dt*1e6/v:.2f} us/col) rc={rc}")
    if stats:
        ph = (ctypes.c_ulonglong * 9)()
        lib.conflux_lu_debug_panel_phase_stats(ph)
        names = ("wait", "load", "update", "publish")
        cols = max(int(ph[8]), 1)
        print("  cycles/col all blocks: " +
              " ".join(f"{k}={ph[i] / cols:.0f}" for i, k in enumerate(names)) +
              " | block 0: " +
              " ".join(f"{k}={ph[4 + i] / cols:.0f}"
                       for i, k in enumerate(names)))
