"""Per-kernel times of the scoring kernels from a rocprofv3 kernel trace of tools/score_rate.py (see its docstring for the
command): every dispatch of k_score / k_compare / k_summary, grouped by kernel and grid size (a full slice of 8 192 positions is
2 048 workgroups; the last slice is shorter), with median, min and max of End - Start and the bytes per second of the rows a
dispatch reads (18 688 B per position and row).  Prints one JSON line; --append FILE adds it to that file.

    python tools/score_kernel_times.py TRACE_DIR_OR_CSV --label dense|sparse|compare [--append profiles/score_rate_<date>.jsonl]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROW_BYTES = 18688
ROWS_READ = {("k_score", "dense"): 2, ("k_score", "sparse"): 1, ("k_compare", "compare"): 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--label", required=True, choices=("dense", "sparse", "compare"))
    ap.add_argument("--append")
    a = ap.parse_args()
    files = [a.trace] if os.path.isfile(a.trace) else glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.trace}")
    groups = {}
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = next((k for k in ("k_score", "k_compare", "k_summary") if "scsc::" + k in r["Kernel_Name"] or k in r["Kernel_Name"]), None)
                if name is None:
                    continue
                wg = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
                groups.setdefault((name, wg), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"tool": "score_kernel_times", "label": a.label, "kernels": []}
    for (name, wg), us in sorted(groups.items()):
        row = {"kernel": name, "workgroups": wg, "dispatches": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
               "max_us": round(max(us), 2)}
        rows = ROWS_READ.get((name, a.label))
        if rows and name != "k_summary":
            row["positions"] = wg * 4
            row["rows_read_GBps_at_median"] = round(wg * 4 * rows * ROW_BYTES / (statistics.median(us) * 1e-6) / 1e9, 1)
        out["kernels"].append(row)
    line = json.dumps(out)
    if a.append:
        with open(a.append, "a") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    sys.exit(main())
