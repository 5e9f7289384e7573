"""Tube maps against merged code: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo), plain, from 8 sources and at 16
frequencies, rasterised on 256 x 512 and 1 024 x 2 048 lat/lon grids.  Per case, in one process, after the launch: `tubemap` - geoac_fan_tubemap by
HIP events on the context's stream (median, min and max of --reps warm rounds after one untimed round) and its work counters; baselines, all merged
code: `stations` - geoac_fan_stations at the same cell centres (cap 1; one call, 256 x 512 only: the brute-force search of the larger grid is
16 times that), `map` - geoac_fan_map on the same grid, and the launch itself.  For the plain case the cooperative threshold is also varied
(GEOAC_TUBE_COOP; the layers are checked to be the same bits).  Every case is a child process of its own under a time limit; a child that fails
ends the run.
usage: perf_tubemap.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRIDS = {"256x512": dict(origin=(12.0, -20.0), step=(36.0 / 256, 40.0 / 512), n=(256, 512)),
         "1024x2048": dict(origin=(12.0, -20.0), step=(36.0 / 1024, 40.0 / 2048), n=(1024, 2048))}
EDGE_MAX = 2.0
CASES = ("plain", "sources8", "freqs16")
THRESHOLDS = (0, 8, 32, 128, 2**31 - 1)              # 32 is GEOAC_TUBE_COOP_MIN; the last one never walks cooperatively


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def step(case, reps):
    import geoac_amd as G
    import harness as H
    import tubemap_reference as TR
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt = int(np.flatnonzero(ph != ph[0])[0])
    nph = th.size // nt
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    if case == "sources8":
        ctx.set_sources(np.array([[0.0, 28.0 + 0.5 * s, -2.0 + 0.5 * s] for s in range(8)]))
    if case == "freqs16":
        ctx.set_frequencies([float(f"{v:.4g}") for v in np.logspace(np.log10(0.05), np.log10(5.0), 16)])
    ctx.set_angles(th, ph)
    ctx.launch()
    res = dict(case=case, rays=int(th.size), lattice=[nt, nph], edge_max=EDGE_MAX, launch_event_ms=round(ctx.timing()["ms_total"], 2), grids={})
    os.environ.pop("GEOAC_TUBE_COOP", None)
    for gname, grid in GRIDS.items():
        kw = dict(grid, n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=EDGE_MAX, detect_db=-70.0)
        ev = []
        for r in range(reps + 1):
            out = ctx.tubemap(**kw)
            ev.append(ctx.tubemap_timing())
        g = dict(tubemap_event_ms=spread(ev[1:]), walk=ctx.tubemap_stats(), hits=int(out["count"].sum()),
                 share_of_cells_reached=round(float((out["count"][0] >= 1).mean()), 4), layer_MB=round(sum(v.nbytes for v in out.values()) / 1e6, 1))
        mv = []
        for r in range(reps + 1):
            binned = ctx.map(detect_db=-70.0, **grid)
            mv.append(ctx.map_timing())
        g["map_event_ms"] = spread(mv[1:])
        g["share_of_cells_reached_point_binned"] = round(float((binned["count"][0] >= 1).mean()), 4)
        if case == "plain":
            by_thr = {}
            for t in THRESHOLDS:
                os.environ["GEOAC_TUBE_COOP"] = str(t)
                tv = []
                for r in range(reps + 1):
                    alt = ctx.tubemap(**kw)
                    tv.append(ctx.tubemap_timing())
                TR.assert_layers_equal(alt, out, f"threshold {t}")
                by_thr[str(t)] = dict(spread(tv[1:]), cooperative=ctx.tubemap_stats()["cooperative"])
            os.environ.pop("GEOAC_TUBE_COOP", None)
            g["tubemap_event_ms_by_cooperative_threshold"] = by_thr
        if gname == "256x512":
            sp = TR.spec(**kw)
            hits, _, _ = ctx.stations(sta=TR.centres(sp), n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=EDGE_MAX, cap=1)
            g["stations_event_ms_one_call"] = round(ctx.stations_timing(), 1)
            g["stations"] = int(hits.shape[1])
            g["count_equals_station_hits"] = bool(np.array_equal(out["count"].reshape(hits.shape), hits.astype(np.uint64)))
            g["stations_over_tubemap"] = round(g["stations_event_ms_one_call"] / g["tubemap_event_ms"]["median"], 1)
        g["tubemap_over_launch"] = round(g["tubemap_event_ms"]["median"] / res["launch_event_ms"], 4)
        res["grids"][gname] = g
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tubemap_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_tubemap.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) rasterised on lat/lon grids over lat 12 .. 48, lon -20 .. 20; library {G.build_id()}",
             "# tubemap_event_ms / map_event_ms: HIP events on the context's stream around geoac_fan_tubemap / geoac_fan_map, median / min / max of "
             f"{a.reps} warm rounds after one untimed round;",
             "# stations_event_ms_one_call: geoac_fan_stations at the cell centres of the 256 x 512 grid (cap 1), one call; walk: the tube map's work counters;",
             "# tubemap_event_ms_by_cooperative_threshold: GEOAC_TUBE_COOP varied (32 is the built-in GEOAC_TUBE_COOP_MIN, 2147483647 never walks cooperatively), same bits checked"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_tubemap: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
