"""Level stations against what they replace: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) launched with four levels
(10 / 20 / 35 / 110 km), plain and from 8 sources, searched for R = 64 / 1 024 / 16 384 stations on rings of 0.2 .. 3 degrees around the source, the
stations dealt to the four levels in turn.  Per case, in one process, after the launch: `call` - geoac_fan_level_stations by HIP events and by host
wall clock (the call + a stream sync), `lists_fetch` - hits and rows to the host; against the parent interface: `fetch_levels` - counts and crossing
records to the host - and `host_search` - tests/lstation_reference.py on the fetched tables (plain, R = 64; one round); and the launch itself.
Median, min and max of --reps warm rounds after one untimed round.  Every case is a child process of its own under a time limit; a child that
fails ends the run.
usage: perf_lstations.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("plain", "sources8")
STATIONS = (64, 1024, 16384)
LEVELS = [10.0, 20.0, 35.0, 110.0]
LVL_CAP, CAP, ORD_MAX = 8, 16, 1


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def rings(n, lat0=30.0, lon0=0.0):
    """n stations on rings of 64 around the source, radii from 0.2 to 3 degrees of arc (R = 64: one ring of 1 degree); level k % 4"""
    k = np.arange(n)
    az = (k % 64) * (2.0 * np.pi / 64)
    rad = np.full(n, 1.0) if n <= 64 else 0.2 + 2.8 * (k // 64) / max(1, n // 64 - 1)
    return np.stack([lat0 + rad * np.cos(az), lon0 + rad * np.sin(az) / np.cos(np.radians(lat0))], axis=1), (k % len(LEVELS)).astype(np.int32)


def step(case, reps):
    import geoac_amd as G
    import harness as H
    import lstation_reference as LS
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt, nph = 90, 360
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    if case == "sources8":
        ctx.set_sources(np.array([[0.0, 28.0 + 0.5 * s, -2.0 + 0.5 * s] for s in range(8)]))
    ctx.set_levels(LEVELS, cap=LVL_CAP)
    ctx.set_angles(th, ph)
    launch = []
    for r in range(reps + 1):
        ctx.launch()
        launch.append(ctx.timing()["ms_total"])
    spec = G.lstation_spec(nt, nph, phi_periodic=True, ord_max=ORD_MAX, cap=CAP)
    fetch = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        count, lrec = ctx.fetch_levels()
        fetch.append((time.perf_counter() - t0) * 1e3)
    count, lrec = count.reshape((-1,) + count.shape[-2:]), lrec.reshape((-1,) + lrec.shape[-4:])
    legs = ctx.params.bounces + 1
    launch_ms = float(np.median(launch[1:]))
    res = dict(case=case, members=int(lrec.shape[0]), rays=int(lrec.shape[1]), levels=len(LEVELS), legs=legs, branches=legs * 2 * ORD_MAX, cells=(nt - 1) * nph,
               crossing_record_MB=round((lrec.nbytes + count.nbytes) / 1e6, 1), launch_event_ms=spread(launch[1:]), fetch_levels_ms=spread(fetch[1:]), by_stations={})
    for R in STATIONS:
        sta, lv = rings(R)
        ev, wall, lfetch = [], [], []
        for r in range(reps + 1):
            if r == 0:
                ctx.launch()                                           # (a launch of its own: the untimed round forms the branch table, the warm rounds reuse it)
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.geoac_fan_level_stations(ctx._h, ctypes.byref(spec), len(sta), sta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), lv.ctypes.data_as(ctypes.c_void_p)))
            ctx._chk(ctx.lib.geoac_fan_sync(ctx._h))
            t1 = time.perf_counter()
            if r == 0:
                first_event = ctx.level_stations_timing()
            out = ctx.level_stations(spec, sta, lv)                    # (the search again + the fetch of the lists)
            t2 = time.perf_counter()
            ev.append(ctx.level_stations_timing()); wall.append((t1 - t0) * 1e3); lfetch.append((t2 - t1) * 1e3 - ev[-1])
        one = dict(stations=R, list_MB=round(sum(v.nbytes for v in out) / 1e6, 2), hits=int(out[0].sum()), stations_with_hits=int((out[0] > 0).any(axis=0).sum()),
                   most_hits=int(out[0].max()), first_call_event_ms=round(first_event, 3), call_event_ms=spread(ev[1:]), call_wall_ms=spread(wall[1:]),
                   lists_fetch_ms=spread(lfetch[1:]), call_plus_fetch_ms=spread([a + b for a, b in zip(wall[1:], lfetch[1:])]))
        one["cell_tests"] = int(lrec.shape[0]) * R * res["branches"] * res["cells"]
        one["cell_tests_per_us"] = round(one["cell_tests"] / (one["call_event_ms"]["median"] * 1e3), 1)
        one["call_plus_fetch_shorter_than_fetch_levels"] = bool(one["call_plus_fetch_ms"]["median"] < res["fetch_levels_ms"]["median"])
        one["event_share_of_launch"] = round(one["call_event_ms"]["median"] / launch_ms, 4)
        if R <= 64 and lrec.shape[0] == 1:
            t0 = time.perf_counter()
            ref = LS.reference_level_stations(G.EQ_GLOBAL, count, lrec, th, ph, legs, LS.spec(nt, nph, phi_periodic=True, ord_max=ORD_MAX, cap=CAP), sta, lv, block=8)
            one["host_search_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            LS.assert_lists_equal(out, ref)
            one["equals_reference"] = True
        res["by_stations"][str(R)] = one
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstations_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_lstations.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) with levels {LEVELS} km, {LVL_CAP} crossings kept; stations on rings of 0.2 .. 3 degrees "
             f"around the source, dealt to the levels in turn; ord_max {ORD_MAX}, cap {CAP}; library {G.build_id()}",
             "# call_event_ms: HIP events around geoac_fan_level_stations with the branch table in place (first_call_event_ms: the call that forms it); call_wall_ms: the call + a stream sync;",
             "# lists_fetch_ms: hits and rows to the host; fetch_levels_ms: counts and crossing records to the host, what a host search has to move first; host_search_ms:",
             "# tests/lstation_reference.py on those tables (one round); cell_tests = members x stations x branches x cells, the brute-force work of a call;",
             f"# median / min / max of {a.reps} warm rounds after one untimed round; every list that has a host_search_ms was checked bit for bit against the restatement"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_lstations: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
