"""Level loudness maps against merged code: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2 - three legs -, CalcAmp, ToyAtmo) with levels at
10 / 20 / 35 / 110 km, plain and from 8 sources, all four levels mapped with ord_max 1 on a 256 x 512 lat/lon grid.  Per case, in one process,
after the launch: `ampmap` - geoac_fan_level_ampmap - and `ltubemap` - geoac_fan_level_tubemap on the same spec - by HIP events on the context's
stream, the two calls alternating, median, min and max of --reps warm rounds after one round of each reported apart (the first ampmap call follows a
fresh launch and forms the branch table, the first ltubemap call finds it), the walk's work counters of both (they must agree: it is the same walk),
the hits, and the launch itself.  Every case is a child process of its own under a time limit; a child that fails ends the run.
usage: perf_lampmap.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EXTENT = dict(origin=(12.0, -20.0), width=(36.0, 40.0))
GRID = (256, 512)
LEVELS = [10.0, 20.0, 35.0, 110.0]
EDGE_MAX = 2.0
CASES = ("plain", "sources8")


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def step(case, reps):
    import geoac_amd as G
    import harness as H
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
    ctx.launch()                                         # (the second launch is warm; no branch table yet: the first ampmap call below forms it)
    res = dict(case=case, rays=int(th.size), lattice=[nt, nph], levels_km=LEVELS, edge_max=EDGE_MAX, grid=list(GRID), launch_event_ms=round(ctx.timing()["ms_total"], 2))
    shared = dict(origin=EXTENT["origin"], step=(EXTENT["width"][0] / GRID[0], EXTENT["width"][1] / GRID[1]), n=GRID, level_mask=0b1111, n_theta=nt, n_phi=nph,
                  phi_periodic=True, edge_max=EDGE_MAX, ord_max=1)
    os.environ.pop("GEOAC_LTUBE_COOP", None)
    aspec, tspec = G.lampmap_spec(detect_amp=1e-5, **shared), G.ltube_spec(**shared)
    amp_ms, tube_ms, formed = [], [], []
    for r in range(reps + 1):
        ctx._chk(ctx.lib.geoac_fan_level_ampmap(ctx._h, ctypes.byref(aspec)))
        amp_ms.append(ctx.level_ampmap_timing())
        formed.append(ctx.level_ampmap_stats()["table_formed"])
        ctx._chk(ctx.lib.geoac_fan_level_tubemap(ctx._h, ctypes.byref(tspec)))
        tube_ms.append(ctx.level_tubemap_timing())
    assert formed[0] and not any(formed[1:])             # (the warm rounds find the table)
    M = ctx._launch_members()
    shape = (M, len(LEVELS)) + GRID
    cnt, weak, tcnt = (np.empty(shape, dtype=np.uint64) for _ in range(3))
    ramp = np.empty(shape)
    ctx._chk(ctx.lib.geoac_fan_level_ampmap_fetch(ctx._h, G.LAMPMAP["COUNT"], cnt.ctypes.data_as(ctypes.c_void_p)))
    ctx._chk(ctx.lib.geoac_fan_level_ampmap_fetch(ctx._h, G.LAMPMAP["WEAK"], weak.ctypes.data_as(ctypes.c_void_p)))
    ctx._chk(ctx.lib.geoac_fan_level_ampmap_fetch(ctx._h, G.LAMPMAP["RAMP_MAX"], ramp.ctypes.data_as(ctypes.c_void_p)))
    ctx._chk(ctx.lib.geoac_fan_level_tubemap_fetch(ctx._h, G.LTUBE["COUNT"], tcnt.ctypes.data_as(ctypes.c_void_p)))
    walk_a, walk_t = ctx.level_ampmap_stats(), ctx.level_tubemap_stats()
    res.update(ampmap_event_ms=spread(amp_ms[1:]), ampmap_first_call_event_ms=round(amp_ms[0], 3), ltubemap_event_ms=spread(tube_ms[1:]),
               ltubemap_first_call_event_ms=round(tube_ms[0], 3), walk=walk_a, same_walk_as_ltubemap=all(walk_a[k] == walk_t[k] for k in ("triangles", "cooperative", "candidates")),
               usable_hits=int(cnt.sum()), weak_hits=int(weak.sum()), count_plus_weak_equals_ltube_count=bool(np.array_equal(cnt + weak, tcnt)),
               share_of_cells_reached_per_level=[round(float((cnt[0, l] >= 1).mean()), 4) for l in range(len(LEVELS))],
               ramp_max_range=[float(ramp[cnt > 0].min()), float(ramp.max())], layer_MB=round((5 * cnt.nbytes + cnt.nbytes // (2 * M)) / 1e6, 1))
    res["ampmap_over_ltubemap"] = round(res["ampmap_event_ms"]["median"] / res["ltubemap_event_ms"]["median"], 2)
    res["ampmap_over_launch"] = round(res["ampmap_event_ms"]["median"] / res["launch_event_ms"], 4)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lampmap_perf.txt"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_lampmap.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) with levels at 10 / 20 / 35 / 110 km, all four mapped (ord_max 1, both "
             f"directions, det_floor 0, a DETECT layer) on a 256 x 512 lat/lon grid over lat 12 .. 48, lon -20 .. 20; library {G.build_id()}",
             f"# ampmap_event_ms / ltubemap_event_ms: HIP events on the context's stream around geoac_fan_level_ampmap / geoac_fan_level_tubemap on the same spec, the two calls "
             f"alternating in one process, median / min / max of {a.reps} warm rounds after the first of each; the first ampmap call follows a fresh launch and forms the branch table;",
             "# launch_event_ms: the launch (warm) the maps were made of; walk: the work counters of the map's pass 0"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_lampmap: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
