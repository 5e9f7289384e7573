"""what every RK4 epoch of one pass waited for, from a rocprofv3 --kernel-trace CSV of bench.py (hybrid fan: a two-lane and a one-lane k_rk4 launch per epoch).
usage: chunk_reuse_timeline.py <kernel_trace.csv> [chunks = 3] [pass = -1 (the last one)]

A pass starts at its k_init launch.  Within it the k-th two-lane launch (EqGlobalPair), the k-th k_postpass_tab, k_ppfix and k_accum launch belong to
epoch k.  Per epoch with work: when the epoch before ended (the later of its two RK4 launches), when this one started, the gap between the two - and
beside it when k_postpass_tab, k_ppfix and k_accum of the epoch `chunks` back ended, i.e. when the chunk's post-pass had read it and when its sums were done.
Times in ms from the pass's k_init."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
n_chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = int(sys.argv[3]) if len(sys.argv) > 3 else -1
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
starts = [i for i, r in enumerate(rows) if "k_init" in r["Kernel_Name"]]
if not starts:
    sys.exit("no k_init launch in the trace")
lo = starts[which]
later = [i for i in starts if i > lo]
rows = rows[lo:(later[0] if later else len(rows))]
t0 = int(rows[0]["Start_Timestamp"])


def span(r):
    return (int(r["Start_Timestamp"]) - t0) / 1e6, (int(r["End_Timestamp"]) - t0) / 1e6


def of(key, without=None):
    return [span(r) for r in rows if key in r["Kernel_Name"] and not (without and without in r["Kernel_Name"])]


pair, one = of("EqGlobalPair"), of("k_rk4", "EqGlobalPair")
post, fix, acc = of("k_postpass_tab"), of("k_ppfix"), of("k_accum")
print(f"# pass {which}: {len(pair)} two-lane and {len(one)} one-lane k_rk4 launches, {len(post)} k_postpass_tab, {len(fix)} k_ppfix, {len(acc)} k_accum; chunks in rotation: {n_chunks}")
print("# epoch  prev RK4 end      start  gap [ms]  of it before ppfix(e-n) / accum(e-n) ended [ms] |  of epoch e - n: postpass_tab end  ppfix end  accum end")


def epoch_end(e):
    t = pair[e][1]
    for a, b in one:                      # the one-lane launch that ran beside it
        if a < pair[e][1] and b > pair[e][0]:
            t = max(t, b)
    return t


def end(lst, e):
    return f"{lst[e][1]:9.2f}" if 0 <= e < len(lst) else "        -"


tot_gap = tot_chunk = tot_fix = 0.0
worst = 0.0
for e in range(1, len(pair)):
    a, b = pair[e]
    if b - a < 0.05:                       # the launch behind the last epoch: it finds finished rays only
        continue
    prev = epoch_end(e - 1)
    gap = a - prev
    # what of the gap the chunk can explain: from the previous epoch's end to the end of k_ppfix / k_accum of epoch e - n, as far as this launch had not started by then
    x = e - n_chunks
    waited = max(0.0, min(a, acc[x][1]) - prev) if 0 <= x < len(acc) else 0.0
    waited_fix = max(0.0, min(a, fix[x][1]) - prev) if 0 <= x < len(fix) else 0.0
    tot_gap += gap
    tot_chunk += waited
    tot_fix += waited_fix
    worst = max(worst, waited)
    print(f"  {e:3d}   {prev:9.2f}  {a:9.2f}  {gap:7.3f}   {waited_fix:7.3f} / {waited:7.3f}                                |                  {end(post, x)}      {end(fix, x)}  {end(acc, x)}")
last = max(b for _, b in pair + one + post + fix + acc)
print(f"# gaps between the RK4 epochs: {tot_gap:.3f} ms in all; of that before k_ppfix(e - n) ended {tot_fix:.3f} ms, before k_accum(e - n) ended {tot_chunk:.3f} ms (the longest {worst:.3f} ms); "
      f"RK4 launches {sum(b - a for a, b in pair):.2f} ms, last kernel of the pass ends at {last:.2f} ms")
