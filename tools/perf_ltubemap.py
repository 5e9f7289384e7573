"""Level tube maps against merged code: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2 - three legs -, CalcAmp, ToyAtmo) with levels at
10 / 20 / 35 / 110 km, plain and from 8 sources, rasterised with ord_max 1 on 256 x 512 and 1 024 x 2 048 lat/lon grids.  Per case, in one
process, after the launch: `ltubemap` - geoac_fan_level_tubemap by HIP events on the context's stream (median, min and max of --reps warm rounds
after one round reported apart) and its work counters.  The round reported apart is the first call on a grid: on the 256 x 512 grid the fan is
launched again just before it, so that the call forms the branch table itself (`first_call_table_formed` says whether it did); on the
1 024 x 2 048 grid it finds the table and only grows its layers.  Baselines, all merged code: `level_stations` -
geoac_fan_level_stations at the 16 384 cell centres of a 128 x 128 grid of the same extent, the four levels in turn (cap 1; one warm call, by HIP
events), `fetch_levels` - the crossing records to the host (wall clock, one warm call), and the launch itself.  Every case is a child process of
its own under a time limit; a child that fails ends the run.
usage: perf_ltubemap.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
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

EXTENT = dict(origin=(12.0, -20.0), width=(36.0, 40.0))
GRIDS = {"256x512": (256, 512), "1024x2048": (1024, 2048)}
STATION_GRID = (128, 128)
LEVELS = [10.0, 20.0, 35.0, 110.0]
EDGE_MAX = 2.0
CASES = ("plain", "sources8")


def grid(n):
    return dict(origin=EXTENT["origin"], step=(EXTENT["width"][0] / n[0], EXTENT["width"][1] / n[1]), n=n)


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def step(case, reps):
    import geoac_amd as G
    import harness as H
    import ltubemap_reference as LT
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt = int(np.flatnonzero(ph != ph[0])[0])
    nph = th.size // nt
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    if case == "sources8":
        ctx.set_sources(np.array([[0.0, 28.0 + 0.5 * s, -2.0 + 0.5 * s] for s in range(8)]))
    ctx.set_levels(LEVELS)
    ctx.set_angles(th, ph)
    ctx.launch()
    res = dict(case=case, rays=int(th.size), lattice=[nt, nph], levels_km=LEVELS, edge_max=EDGE_MAX, launch_event_ms=round(ctx.timing()["ms_total"], 2), grids={})
    ctx.fetch_levels()
    t0 = time.perf_counter()
    count, lrec = ctx.fetch_levels()
    res["fetch_levels_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["crossing_records_MB"] = round((count.nbytes + lrec.nbytes) / 1e6, 1)
    del count, lrec
    lattice = dict(n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=EDGE_MAX, ord_max=1)
    # the brute-force baseline: one station per centre of a 128 x 128 grid, the four levels in turn
    ssp = LT.spec(level_mask=1, **lattice, **grid(STATION_GRID))
    sta = LT.centres(ssp)
    level_of = np.arange(len(sta)) % len(LEVELS)
    for r in range(2):
        hits, _ = ctx.level_stations(sta=sta, level_of=level_of, cap=1, **lattice)
        res["level_stations_event_ms_one_call"] = round(ctx.level_stations_timing(), 1)
    res["level_stations"] = int(hits.shape[1])
    # ... and the same centres through the map: its COUNT is their hits
    small = ctx.level_tubemap(level_mask=0b1111, **lattice, **grid(STATION_GRID))
    per_level = small["count"].reshape(small["count"].shape[0], len(LEVELS), -1)
    res["count_equals_level_station_hits"] = bool(np.array_equal(per_level[:, level_of, np.arange(len(sta))], hits.astype(np.uint64)))
    os.environ.pop("GEOAC_LTUBE_COOP", None)
    for gname, n in GRIDS.items():
        spec = G.ltube_spec(level_mask=0b1111, **lattice, **grid(n))
        if gname == "256x512":
            ctx.launch()                                 # a fresh launch: no branch table yet, the first call below forms it
        ev, formed = [], []
        for r in range(reps + 1):
            ctx._chk(ctx.lib.geoac_fan_level_tubemap(ctx._h, ctypes.byref(spec)))
            ev.append(ctx.level_tubemap_timing())
            formed.append(ctx.level_tubemap_stats()["table_formed"])
        assert not any(formed[1:])                       # (the warm rounds find the table)
        M = ctx._launch_members()
        cnt = np.empty((M, len(LEVELS)) + n, dtype=np.uint64)
        ctx._chk(ctx.lib.geoac_fan_level_tubemap_fetch(ctx._h, G.LTUBE["COUNT"], cnt.ctypes.data_as(ctypes.c_void_p)))
        g = dict(ltubemap_event_ms=spread(ev[1:]), first_call_event_ms=round(ev[0], 3), first_call_table_formed=bool(formed[0]), walk=ctx.level_tubemap_stats(), hits=int(cnt.sum()),
                 share_of_cells_reached_per_level=[round(float((cnt[0, l] >= 1).mean()), 4) for l in range(len(LEVELS))],
                 layer_MB=round((4 * cnt.nbytes + cnt.nbytes // (2 * M)) / 1e6, 1))
        g["level_stations_16384_over_ltubemap"] = round(res["level_stations_event_ms_one_call"] / g["ltubemap_event_ms"]["median"], 2)
        g["fetch_levels_over_ltubemap"] = round(res["fetch_levels_wall_ms"] / g["ltubemap_event_ms"]["median"], 2)
        g["ltubemap_over_launch"] = round(g["ltubemap_event_ms"]["median"] / res["launch_event_ms"], 4)
        res["grids"][gname] = g
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltubemap_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_ltubemap.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) with levels at 10 / 20 / 35 / 110 km, all four rasterised (ord_max 1, both "
             f"directions) on lat/lon grids over lat 12 .. 48, lon -20 .. 20; library {G.build_id()}",
             f"# ltubemap_event_ms: HIP events on the context's stream around geoac_fan_level_tubemap, median / min / max of {a.reps} warm rounds after the first call on the grid; "
             "first_call_event_ms: that first call - on the 256 x 512 grid it follows a fresh launch and forms the branch table (first_call_table_formed), on the other it finds the table;",
             "# level_stations_event_ms_one_call: geoac_fan_level_stations at the 16 384 cell centres of a 128 x 128 grid of the same extent (cap 1), one warm call; "
             "fetch_levels_wall_ms: the crossing records to the host, wall clock, one warm call; walk: the map's work counters"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_ltubemap: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
