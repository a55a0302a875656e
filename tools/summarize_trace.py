"""Durations and gaps of consecutive launches of one kernel in a rocprofv3 --kernel-trace output directory.

    python tools/summarize_trace.py DIR                       the exact-order fronts of the last call (k_sor_exact, last third)
    python tools/summarize_trace.py DIR k_sor_rbp+ModelElin4 200
                                                              the last 200 launches whose name contains every +-separated text:
                                                              duration, and the gap from one launch's end to the next launch's begin
"""
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
name = sys.argv[2] if len(sys.argv) > 2 else "k_sor_exact"
rows = [r for r in csv.DictReader(open(f)) if all(part in r["Kernel_Name"] for part in name.split("+"))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
if len(sys.argv) > 3:
    rows = rows[-int(sys.argv[3]):]
else:
    n = len(rows) // 3
    rows = rows[2 * n:]  # last call
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
gaps = [(int(rows[i + 1]["Start_Timestamp"]) - int(rows[i]["End_Timestamp"])) / 1e3 for i in range(len(rows) - 1)]
med = lambda v: sorted(v)[len(v) // 2]
print("launches", len(d), "sum_us %.1f" % sum(d), "span_us %.1f" % ((int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])) / 1e3),
      "mean gap %.2f" % (sum(gaps) / len(gaps)))
print("duration_us mean %.2f median %.2f min %.2f max %.2f" % (sum(d) / len(d), med(d), min(d), max(d)))
print("gap_us      mean %.2f median %.2f min %.2f max %.2f  (%d gaps)" % (sum(gaps) / len(gaps), med(gaps), min(gaps), max(gaps), len(gaps)))
if len(sys.argv) <= 3:
    for i in range(0, len(d), 6):
        print("m=%3d.." % i, " ".join("%5.1f" % x for x in d[i:i + 6]))
print("VGPR", rows[0].get("VGPR_Count"), "LDS", rows[0].get("LDS_Block_Size"), "grid", rows[0].get("Grid_Size"), rows[0].get("Workgroup_Size"))
