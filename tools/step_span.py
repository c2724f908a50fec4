"""Per step of the sis loop (t = step mod 10), from a rocprofv3 kernel trace (+ its memory-copy trace) of bench.py: the
time no kernel runs, the span from the step's D2H copy (sis.py: `head = ... .cpu()`) to the first gemm_split_kernel - the
stretch the packing plan's index ops fill, paced by the host -, the kernels launched inside that span, and the time in ATen's
float add (the blocks' residual adds; the embedding's wte + wpe is one more a step).  A step ends at its fused call.

    python3 tools/step_span.py <kernel_trace.csv> [memory_copy_trace.csv] [steps per loop = 10]

Without the copy trace the span starts at the end of the last kernel before the copy (group_contexts' tail: the stack
of four words), which is at most the copy's few microseconds early."""
import csv
import sys
from collections import defaultdict

trace = sys.argv[1]
copies = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].isdigit() else None
loop = int(sys.argv[-1]) if sys.argv[-1].isdigit() else 10
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
               for r in csv.DictReader(open(trace, newline=""))))
d2h = []
if copies:
    for r in csv.DictReader(open(copies, newline="")):
        if "DEVICE_TO_HOST" in r.get("Direction", "").upper():
            d2h.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    d2h.sort()
steps, cur = [], []
for r in rows:
    cur.append(r)
    if "fused_step_kernel" in r[2] or "chunk_stats_small_kernel" in r[2]:
        steps.append(cur)
        cur = []
acc = defaultdict(lambda: defaultdict(float))
prev_end = None
for k, st in enumerate(steps):
    lo, hi = (prev_end if prev_end is not None else st[0][0]), st[-1][1]
    prev_end = hi
    if k == 0:
        continue  # (its start is the process's, not a step's)
    a = acc[k % loop]
    a["n"] += 1
    a["wall_us"] += (hi - lo) * 1e-3
    busy, end = 0, lo
    for s, e, _ in st:
        if e > end:
            busy += e - max(s, end)
            end = e
    a["idle_us"] += (hi - lo - busy) * 1e-3
    a["launches"] += len(st)
    first = next((i for i, r in enumerate(st) if "gemm_split_kernel" in r[2]), None)
    if first is not None:
        t_split = st[first][0]
        mine = [c for c in d2h if lo <= c[0] < t_split]
        if mine:
            t0 = mine[-1][1]
            a["with_copy"] += 1
        else:  # the last kernel that ended before a gap holding the .cpu(): the latest launch before the plan's index ops
            before = [r for r in st[:first] if "stack" in r[2].lower() or "CatArrayBatchedCopy" in r[2]]
            t0 = before[0][1] if before else st[0][1]
        inside = [r for r in st[:first] if r[0] >= t0]
        a["span_us"] += (t_split - t0) * 1e-3
        a["span_launches"] += len(inside)
        a["span_kernel_us"] += sum(e - s for s, e, _ in inside) * 1e-3
    for s, e, n in st:
        if "CUDAFunctor_add<float>" in n:
            a["add_us"] += (e - s) * 1e-3
            a["adds"] += 1
        if "packed_plan" in n:
            a["plan_us"] += (e - s) * 1e-3
print(f"# {trace}: {len(steps)} steps, means per step by t = step mod {loop}"
      f"{'' if copies else ' (no copy trace: span from the kernel before the D2H copy)'}")
print(f"{'t':>3s} {'steps':>5s} {'wall us':>8s} {'idle us':>8s} {'launches':>8s} {'D2H->split us':>13s} {'its launches':>12s} "
      f"{'its kernel us':>13s} {'add<float>':>10s} {'add us':>7s} {'plan us':>7s}")
tot = defaultdict(float)
for t in sorted(acc) + ["all"]:
    a = tot if t == "all" else acc[t]
    n = a["n"]
    print(f"{t!s:>3s} {int(n):5d} {a['wall_us'] / n:8.1f} {a['idle_us'] / n:8.1f} {a['launches'] / n:8.1f} {a['span_us'] / n:13.1f} "
          f"{a['span_launches'] / n:12.1f} {a['span_kernel_us'] / n:13.1f} {a['adds'] / n:10.1f} {a['add_us'] / n:7.1f} {a['plan_us'] / n:7.1f}")
    if t != "all":
        for key, v in a.items():
            tot[key] += v
