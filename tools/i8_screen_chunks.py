#!/usr/bin/env python3
"""Per-chunk launch times of cosine_i8_screen from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py
    python tools/i8_screen_chunks.py DIR [chunks_per_batch = 3]

The screen is launched once per chunk of a batch, in the same order every batch; launch i belongs to chunk i mod
chunks_per_batch.  Prints one JSON line: per chunk the number of launches, the median / min / max duration in microseconds and
the workgroups of the launch, and the median of the per-batch sums."""
import csv
import glob
import json
import statistics
import sys

d = sys.argv[1]
per = int(sys.argv[2]) if len(sys.argv) > 2 else 3
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
rows = [r for r in csv.DictReader(open(f)) if "cosine_i8_screen" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
rows = rows[:len(rows) // per * per]
us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
chunks = []
for c in range(per):
    v = us[c::per]
    chunks.append({"launches": len(v), "median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1),
                   "max_us": round(max(v), 1), "workgroups": int(rows[c]["Grid_Size_X"]) // max(1, int(rows[c]["Workgroup_Size_X"]))})
sums = [sum(us[i:i + per]) for i in range(0, len(us), per)]
print(json.dumps({"trace": f.split("/")[-1], "chunks": chunks, "batch_sum_median_us": round(statistics.median(sums), 1)}))
