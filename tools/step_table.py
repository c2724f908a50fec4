"""Per step of the sis loop (t = new tokens so far, 0 .. 9), from a rocprofv3 kernel trace of bench.py: rows fed to the body
(from c_attn's grid: 128-row tiles x 18 column tiles, or 64-row tiles x 36 where the kernel's name carries the small form's
geometry, `Geom<1, 4, ..>`; so rounded up to the tile; 0 where c_attn ran the library GEMM), GEMM time, split launches in
the small form,
attention time and which attention kernel ran, ATen elementwise / copy time, launches.  A step ends at its fused call.

    python3 tools/step_table.py <kernel_trace.csv> [steps per loop = 10]"""
import csv
import re
import sys
from collections import defaultdict

trace = sys.argv[1]
loop = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = sorted(csv.DictReader(open(trace, newline="")), key=lambda r: int(r["Start_Timestamp"]))
steps, cur = [], []
for r in rows:
    cur.append(r)
    n = r["Kernel_Name"]
    if "fused_step_kernel" in n or "chunk_stats_small_kernel" in n:
        steps.append(cur)
        cur = []
acc = defaultdict(lambda: defaultdict(float))
for k, st in enumerate(steps):
    a = acc[k % loop]
    a["n"] += 1
    first_split = True
    for r in st:
        n, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        a["launches"] += 1
        if "gemm_split_kernel" in n or n.startswith("Cijk_") or n.startswith("Custom_Cijk_") or "void Cijk_" in n:
            a["gemm_us"] += us
            if "gemm_split_kernel" in n:
                a["split_launches"] += 1
                geom = re.search(r"Geom<(\d+), (\d+)", n)  # row fragments per wave, column fragments per block
                mf, nf = (int(geom.group(1)), int(geom.group(2))) if geom else (2, 8)
                a["small_launches"] += (mf, nf) != (2, 8)
                if first_split:  # c_attn of the first block: N = 2304
                    grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
                    wg = grid // max(int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"]), 1)
                    a["rows"] += wg / (2304 // (16 * nf)) * 64 * mf
                    first_split = False
            else:
                a["lib_gemm_launches"] += 1
        elif "short_attention_packed" in n:
            a["attn_us"] += us
            a["packed_attn"] += 1
        elif "short_attention" in n or "slab_attention" in n:
            a["attn_us"] += us
            a["padded_attn"] += 1
        elif "at::native" in n:
            a["aten_us"] += us
            a["aten_launches"] += 1
            if "copy" in n.lower():
                a["aten_copy_launches"] += 1
print(f"# {trace}: {len(steps)} steps, means per step by t = step mod {loop}; ATen = at::native kernels (elementwise, copies, LayerNorm)")
print(f"{'t':>2s} {'steps':>5s} {'rows<=':>7s} {'GEMM us':>9s} {'split':>6s} {'small':>6s} {'lib':>5s} {'attn us':>8s} {'packed':>6s} {'padded':>6s} "
      f"{'ATen us':>8s} {'ATen':>6s} {'copies':>6s} {'launches':>8s}")
tot = defaultdict(float)
for t in sorted(acc):
    a = acc[t]
    n = a["n"]
    print(f"{t:2d} {int(n):5d} {a['rows'] / n:7.0f} {a['gemm_us'] / n:9.1f} {a['split_launches'] / n:6.1f} {a['small_launches'] / n:6.1f} {a['lib_gemm_launches'] / n:5.1f} "
          f"{a['attn_us'] / n:8.1f} {a['packed_attn'] / n:6.1f} {a['padded_attn'] / n:6.1f} {a['aten_us'] / n:8.1f} "
          f"{a['aten_launches'] / n:6.1f} {a['aten_copy_launches'] / n:6.1f} {a['launches'] / n:8.1f}")
    for k, v in a.items():
        tot[k] += v
n = tot["n"]
print(f"{'all':>2s} {int(n):5d} {tot['rows'] / n:7.0f} {tot['gemm_us'] / n:9.1f} {tot['split_launches'] / n:6.1f} {tot['small_launches'] / n:6.1f} {tot['lib_gemm_launches'] / n:5.1f} "
      f"{tot['attn_us'] / n:8.1f} {tot['packed_attn'] / n:6.1f} {tot['padded_attn'] / n:6.1f} {tot['aten_us'] / n:8.1f} "
      f"{tot['aten_launches'] / n:6.1f} {tot['aten_copy_launches'] / n:6.1f} {tot['launches'] / n:8.1f}")
