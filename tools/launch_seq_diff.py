#!/usr/bin/env python3
"""Do two runs launch the same kernels, with the same shapes, in the same order?

    rocprofv3 --kernel-trace -d OLD -o t --output-format csv -- \
        python bench.py --gpus 1 --N 4096 --steps 2 --warmup 1
    (the same with the other build into NEW)
    python tools/launch_seq_diff.py OLD/t_kernel_trace.csv NEW/t_kernel_trace.csv

Compares the sequence of (kernel name as tools/gap_from_trace.py shortens it,
grid x/y/z, workgroup x/y/z) in host dispatch order, i.e. sorted by the
trace's Dispatch_Id.  A trace without that column is compared per queue, in
the order of its rows, and the output says so.  Timestamps play no part:
kernels of two streams may start in either order, the host enqueues them in
one.  Exits 0 on identity; otherwise prints the first difference and exits 1.
"""
import csv
import sys
from collections import defaultdict

from gap_from_trace import short

DIMS = [p + a for p in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ"]


def sequences(path):
    """{queue or 'all': [(name, grid..., workgroup...)]}, by dispatch id"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    launch = [(short(r["Kernel_Name"]),) + tuple(int(r[d]) for d in DIMS)
              for r in rows]
    if rows and "Dispatch_Id" in rows[0]:
        order = sorted(range(len(rows)),
                       key=lambda i: int(rows[i]["Dispatch_Id"]))
        return {"all": [launch[i] for i in order]}, True
    per_queue = defaultdict(list)
    for r, l in zip(rows, launch):
        per_queue[r.get("Queue_Id", "?")].append(l)
    # queue ids differ between processes: pair the queues by first use
    return {i: q for i, q in enumerate(per_queue.values())}, False


def main(old_path, new_path):
    (old, by_id), (new, by_id2) = sequences(old_path), sequences(new_path)
    if not (by_id and by_id2):
        print("no Dispatch_Id column: comparing per queue, in row order")
    if sorted(old) != sorted(new):
        print("queues: %d against %d" % (len(old), len(new)))
        return 1
    total = 0
    for q in sorted(old):
        a, b = old[q], new[q]
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                print("queue %s, launch %d differs:\n  old %s\n  new %s" %
                      (q, i, x, y))
                return 1
        if len(a) != len(b):
            longer = a if len(a) > len(b) else b
            print("queue %s: %d launches against %d; first extra: %s" %
                  (q, len(a), len(b), longer[min(len(a), len(b))]))
            return 1
        total += len(a)
    print("identical: %d launches" % total)
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
