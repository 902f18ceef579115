#!/bin/bash
# per-dispatch kernel durations of a command (rocprofv3 --kernel-trace), condensed: one line per dispatch of the small
# kernels, aggregated lines for the rest.   usage: tools/trace_kernels.sh <tag> -- python3 ...
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=$1; shift; shift
OUT=$R/gpurun_out/trace_$TAG
rm -rf "$OUT"; mkdir -p "$OUT"

rocprofv3 --kernel-trace --output-format csv -d "$OUT" -- "$@" > "$OUT/cmd.log" 2>&1
cd "$R"
python3 - "$OUT" <<'PY'
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/*/*_kernel_trace.csv")[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
# last complete pass.  A pass ends with the host waiting for both streams, so the next one's first kernel starts after every kernel so
# far has ended (an idle point); k_sum_dnode runs once per pass (NSUM times in a split / sharded pass), possibly on the side stream
# beside the predictive kernel, so it need not be the last to start.  Passes: cut at the idle points that follow NSUM k_sum_dnode.
import os
nsum = int(os.environ.get("NSUM", "1"))
cuts, seen, busy_until = [0], 0, 0
for i, r in enumerate(rows):
    if i and seen >= nsum and int(r["Start_Timestamp"]) >= busy_until:
        cuts.append(i); seen = 0
    seen += r["Kernel_Name"].startswith("k_sum_dnode")
    busy_until = max(busy_until, int(r["End_Timestamp"]))
if seen >= nsum: cuts.append(len(rows))
seg = rows[cuts[-2]: cuts[-1]] if len(cuts) >= 2 else rows
t0 = int(seg[0]["Start_Timestamp"])
prev_end = t0
# +gap: from the latest end so far to this start; negative where the kernel starts beside one that is still running (the side stream)
for r in seg:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print("%9.1f us  +gap %6.1f  dur %8.1f us  queue %s  grid %9s wg %4s  %s" % ((s - t0) / 1e3, (s - prev_end) / 1e3, (e - s) / 1e3, r.get("Queue_Id", "?"), r.get("Grid_Size", r.get("Grid_Size_X")), r.get("Workgroup_Size", r.get("Workgroup_Size_X")), r["Kernel_Name"][:70]))
    prev_end = max(prev_end, e)
print("pass: %.1f us from first start to last end" % ((prev_end - t0) / 1e3))
PY
