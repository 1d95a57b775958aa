"""Two rocprofv3 --kernel-trace outputs (<name>_results.db) of the same program on two builds: do they hold the same launches?
    python3 tools/probes/compare_kernel_traces.py <a_results.db> <b_results.db> [label]
Per stream (numbered by first appearance, since ids differ between processes): kernel name with template arguments, grid and workgroup size,
in start order.  A stream whose ORDER differs but whose launches are the same multiset is reported as such (two host threads enqueue on the
stream that B1 and K share, so one build differs from itself there)."""
import sqlite3
import sys
from collections import Counter, defaultdict


def launches(db):
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    first = lambda *names: next(n for n in names if n in cols)
    sid, gx, wx = first("stream_id", "queue_id"), first("grid_x", "grid_size_x"), first("workgroup_x", "workgroup_size_x")
    opt = lambda *names: next((n for n in names if n in cols), "0")
    gy, gz = opt("grid_y", "grid_size_y"), opt("grid_z", "grid_size_z")
    streams, order = defaultdict(list), {}
    for s, name, x, y, z, w in c.execute(f"select {sid}, name, {gx}, {gy}, {gz}, {wx} from kernels order by start"):
        streams[order.setdefault(s, len(order))].append((name, f"{x}x{y}x{z}", w))
    return streams


a, b = launches(sys.argv[1]), launches(sys.argv[2])
label = sys.argv[3] if len(sys.argv) > 3 else "trace"
same_all = True
print(f"{label}: {sum(map(len, a.values()))} launches on {len(a)} streams against {sum(map(len, b.values()))} on {len(b)}")
for s in sorted(set(a) | set(b)):
    la, lb = a.get(s, []), b.get(s, [])
    if la == lb:
        verdict = "same launches, same order"
    elif Counter(la) == Counter(lb):
        verdict = "same launches, ORDER differs (first at position %d)" % next(i for i, (x, y) in enumerate(zip(la, lb)) if x != y)
    else:
        verdict, same_all = "DIFFERENT launches", False
        for k, n in ((Counter(la) - Counter(lb)) + (Counter(lb) - Counter(la))).most_common(8):
            print(f"      {n:4d} x {k[0][:90]} grid {k[1]} wg {k[2]}  (a {Counter(la)[k]}, b {Counter(lb)[k]})")
    print(f"  stream {s}: {len(la):5d} / {len(lb):5d} launches, {len(set(x[0] for x in la)):3d} distinct kernels: {verdict}")
print(f"{label}:", "the two builds launch the same kernels with the same grids and workgroup sizes" if same_all else "LAUNCH LISTS DIFFER")
