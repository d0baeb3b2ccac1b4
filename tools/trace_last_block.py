"""Per-launch times around the last block's attention from a rocprofv3 kernel trace: usage: python tools/trace_last_block.py <rocprofv3 output dir> <depth>; medians over the forwards of the run (the first is warm-up)"""
import csv, glob, sys, statistics, re
d, depth = sys.argv[1], int(sys.argv[2])
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: re.sub(r"^void ", "", r["Kernel_Name"])[:100]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
A = [i for i, r in enumerate(rows) if "attn_fused_kernel" in r["Kernel_Name"]]
steps = len(A) // depth
print(f"{len(rows)} dispatches, {len(A)} attention launches = {steps} forwards of depth {depth}")
for off in range(-1, 6):
    ds, nm = [], None
    for s in range(1, steps):          # the first forward is warm-up
        i = A[depth * s + depth - 1] + off
        if i < len(rows):
            ds.append(dur(rows[i])); nm = name(rows[i])
    if ds:
        print(f"  last attention {off:+d}: median {statistics.median(ds):7.1f} us  min {min(ds):7.1f}  n {len(ds):3d}  {nm}")
# and one earlier block for comparison (block depth-2: attention, proj, norm2+Mlp)
for off in range(0, 3):
    ds, nm = [], None
    for s in range(1, steps):
        i = A[depth * s + depth - 2] + off
        ds.append(dur(rows[i])); nm = name(rows[i])
    print(f"  block {depth-2} attention {off:+d}: median {statistics.median(ds):7.1f} us  min {min(ds):7.1f}  n {len(ds):3d}  {nm}")
