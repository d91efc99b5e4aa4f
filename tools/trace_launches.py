"""Per-launch times of selected kernels from a rocprofv3 kernel trace (`--kernel-trace --output-format csv`), told apart by
call site: launches are grouped by (kernel, grid size, kernel before, kernel after) in stream order, which names the place
in the step a launch comes from when the run was eager.

    python tools/trace_launches.py <kernel_trace.csv> gather2_kernel copy_rows_kernel [--steps 35]
"""
import argparse
import csv
import re
import statistics
import sys


def short(name: str) -> str:
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"\(.*$", "", name)[:72]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--steps", type=int, default=0, help="steps in the run: prints launches per step next to the count")
    a = ap.parse_args()
    with open(a.trace, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    groups = {}
    for i, r in enumerate(rows):
        if not any(p in names[i] for p in a.patterns):
            continue
        key = (names[i], int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), names[i - 1] if i else "-",
               names[i + 1] if i + 1 < len(rows) else "-")
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'count':>6} {'/step':>6} {'mean us':>8} {'min':>7} {'max':>7} {'sd':>6}  kernel [grid]  <- before  -> after")
    for key, d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        sd = statistics.pstdev(d) if len(d) > 1 else 0.0
        per = f"{len(d) / a.steps:6.2f}" if a.steps else "     -"
        print(f"{len(d):6d} {per} {statistics.mean(d):8.2f} {min(d):7.2f} {max(d):7.2f} {sd:6.2f}  {key[0]} [{key[1]}]  <- {key[2]}  -> {key[3]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
