#!/usr/bin/env python3
"""Serial stretch between two panel chains, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- \
        python bench.py --gpus 1 --steps 3 --warmup 1
    python tools/gap_from_trace.py DIR/t_kernel_trace.csv

For every pair of consecutive panel chains (a chain = the run of
k_panel_factor / k_panel_glue_* launches of one panel) the gap runs from the
end of the chain's last kernel to the start of the next chain's first
k_panel_factor.  Printed per factorization step (averaged over the traced
factorizations): the gap, the time inside it that is covered by each kernel
family other than the capped trailing GEMM of the previous step, and the
part of the gap in which none of those kernels runs ("idle": host work,
launch latency, copies the trace does not show).  Trailing-GEMM launches
(k_dgemm_mfma<GemmW8>, in the table k_dgemm_f64_w8, with the capped grid) are
reported separately because they overlap the stretch without being part of it.
"""
import csv
import sys
from collections import defaultdict


# the editions of k_dgemm_mfma<Cfg> are reported under the names these kernels
# had before they became one template, so that traces from before and after,
# and the tables in profiles/, read alike
GEMM_EDITIONS = {"GemmW4": "k_dgemm_f64", "GemmW8": "k_dgemm_f64_w8",
                 "GemmBm256": "k_dgemm_f64_bm256",
                 "GemmW8NT": "k_dgemm_f64_w8_nt"}


def short(name):
    n = name.split("(")[0].replace("void ", "").replace("ck::", "")
    base, _, args = n.partition("<")
    if base == "k_dgemm_mfma":
        return GEMM_EDITIONS.get(args.rstrip("> "), base)
    return base


def main(path, nt=32):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         short(r["Kernel_Name"]), int(r["Grid_Size_X"]),
                         int(r["Workgroup_Size_X"])))
    rows.sort()
    # the leaf is k_panel_factor or, since r06, k_panel_factor_reg
    leaf = ("k_panel_factor", "k_panel_factor_reg")
    panel = leaf + ("k_panel_glue_prep", "k_panel_glue_update")
    # chains: split the panel-kernel sequence where the right solve (main
    # stream, always inside the stretch) lies between two panel kernels; the
    # left solve does not qualify: with the one-rank direct step its rest
    # runs next to the first leaves of the next chain
    chains, cur = [], []
    last_trsm = -1
    for i, (s, e, n, g, w) in enumerate(rows):
        if n.startswith("k_trsm_right"):
            last_trsm = i
        if n in panel:
            if cur and last_trsm > cur[-1]:
                chains.append(cur)
                cur = []
            cur.append(i)
    if cur:
        chains.append(cur)
    per_step = defaultdict(list)
    for ci in range(len(chains) - 1):
        step = ci % nt
        if step == nt - 1:
            continue  # next chain belongs to the next factorization
        t0 = max(rows[i][1] for i in chains[ci])
        nxt = [i for i in chains[ci + 1] if rows[i][2] in leaf]
        t1 = rows[nxt[0]][0]
        fam = defaultdict(float)
        segs = []
        for (s, e, n, g, w) in rows:
            if e <= t0 or s >= t1 or n in panel:
                continue
            a, b = max(s, t0), min(e, t1)
            capped = n == "k_dgemm_f64_w8" and g // w == 432
            key = "gemm_capped(prev step)" if capped else n
            fam[key] += (b - a) / 1e3
            if not capped:
                segs.append((a, b))
        segs.sort()
        busy, end = 0, t0
        for a, b in segs:
            if b > end:
                busy += b - max(a, end)
                end = b
        per_step[step].append(((t1 - t0) / 1e3, (t1 - t0 - busy) / 1e3, fam))
    names = sorted({k for v in per_step.values() for (_, _, f) in v for k in f})
    print("step,gap_us,idle_us," + ",".join(n + "_us" for n in names))
    tot = defaultdict(float)
    for step in sorted(per_step):
        v = per_step[step]
        gap = sum(x[0] for x in v) / len(v)
        idle = sum(x[1] for x in v) / len(v)
        fams = [sum(x[2].get(n, 0.0) for x in v) / len(v) for n in names]
        tot["gap"] += gap
        tot["idle"] += idle
        for n, x in zip(names, fams):
            tot[n] += x
        print(f"{step},{gap:.0f},{idle:.0f}," +
              ",".join(f"{x:.0f}" for x in fams))
    print("sum_per_factorization_ms,%.2f,%.2f," % (tot["gap"] / 1e3,
                                                  tot["idle"] / 1e3) +
          ",".join("%.2f" % (tot[n] / 1e3) for n in names))


if __name__ == "__main__":
    main(sys.argv[1])
