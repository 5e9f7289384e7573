"""What level crossings cost: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) with L = 0 / 1 / 4 / 8 levels set, in one process
on one context.  Per L: the launch by HIP events (timing()["ms_total"]), median / min / max of --reps warm rounds after one untimed round, the crossings
found, the largest count of a (ray, level) pair against the cap, and the fetch of counts and records to the host.  L = 0 comes first and last: the
two figures bracket the drift of the session.
usage: perf_levels.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS = {0: [], 1: [35.0], 4: [10.0, 20.0, 35.0, 110.0], 8: [5.0, 10.0, 20.0, 35.0, 50.0, 80.0, 100.0, 110.0]}
CAP = 8


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_perf.txt"))
    a = ap.parse_args()
    import geoac_amd as G
    import harness as H
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_angles(th, ph)
    lines = [f"# tools/perf_levels.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo), cap {CAP}; library {G.build_id()}",
             f"# launch_ms: HIP events around the whole launch, median / min / max of {a.reps} warm rounds after one untimed round, one process, one context;",
             "# fetch_ms: counts and records to the host (host wall clock).  L = 0 is measured first and last."]
    base = None
    for L in (0, 1, 4, 8, 0):
        ctx.set_levels(LEVELS[L], cap=CAP)
        ms = []
        for r in range(a.reps + 1):
            ctx.launch()
            ms.append(ctx.timing()["ms_total"])
        res = dict(levels=L, z_km=LEVELS[L], launch_ms=spread(ms[1:]), epochs=int(ctx.timing()["epochs"]))
        if base is None:
            base = res["launch_ms"]["median"]
        res["over_L0_first_ms"] = round(res["launch_ms"]["median"] - base, 3)
        if L:
            t0 = time.perf_counter()
            count, rec = ctx.fetch_levels()
            res["fetch_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            res["crossings"] = int(count.sum()); res["largest_count"] = int(count.max()); res["record_MB"] = round(rec.nbytes / 1e6, 1)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    ctx.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
