"""Level refinement at the size of its use: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) launched with four levels
(10 / 20 / 35 / 110 km), plain and from 8 sources, its level-station lists for R = 64 stations on a ring of 1 degree around the source (dealt to
the four levels in turn) refined by geoac_fan_level_refine.  Per case, in one process: the lattice launch by HIP events; per call of the
refinement its launches (the sum of geoac_last_timing over its rounds), its own kernels (HIP events around k_lrf_step / k_lrf_rows), the host wall
clock of the call, the rounds used, the seeds and their statuses.  Every repetition is lattice launch, lists, refinement (the refinement's first
launch invalidates the lists).  Median, min and max of --reps warm repetitions after one untimed one.  Every case is a child process of its own
under a time limit; a child that fails ends the run.
usage: perf_level_refine.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
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

from perf_lstations import LEVELS, LVL_CAP, CAP, ORD_MAX, rings, spread          # noqa: E402  (the case of tools/perf_lstations.py)

CASES = ("plain", "sources8")
STATIONS = 64
SPEC = dict(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2, probe_deg=0.02)


def step(case, reps):
    import geoac_amd as G
    import harness as H
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt, nph = 90, 360
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    if case == "sources8":
        ctx.set_sources(np.array([[0.0, 28.0 + 0.5 * s, -2.0 + 0.5 * s] for s in range(8)]))
    ctx.set_levels(LEVELS, cap=LVL_CAP)
    lspec = G.lstation_spec(nt, nph, phi_periodic=True, ord_max=ORD_MAX, cap=CAP)
    rspec = G.level_refine_spec(**SPEC)
    sta, lv = rings(STATIONS)
    lattice, lists, launches, kernels, wall = [], [], [], [], []
    for r in range(reps + 1):
        ctx.set_angles(th, ph)
        ctx.launch()
        lattice.append(ctx.timing()["ms_total"])
        ctx._chk(ctx.lib.geoac_fan_level_stations(ctx._h, ctypes.byref(lspec), len(sta), sta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), lv.ctypes.data_as(ctypes.c_void_p)))
        lists.append(ctx.level_stations_timing())
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.geoac_fan_level_refine(ctx._h, ctypes.byref(rspec)))
        ctx._chk(ctx.lib.geoac_fan_sync(ctx._h))
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = ctx.level_refine_timing()
        launches.append(ms["launch_ms"]); kernels.append(ms["kernel_ms"])
    # the last repetition's result
    n, it = ctypes.c_int(0), ctypes.c_int(0)
    ctx._chk(ctx.lib.geoac_fan_level_refine_shape(ctx._h, ctypes.byref(n), ctypes.byref(it)))
    rows = np.empty((n.value, G.LRF_STRIDE))
    ctx._chk(ctx.lib.geoac_fan_level_refine_fetch(ctx._h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    st = np.zeros(6, dtype=np.uint64)
    ctx._chk(ctx.lib.geoac_fan_level_refine_stats(ctx._h, st.ctypes.data_as(ctypes.c_void_p)))
    M = 8 if case == "sources8" else 1
    status = np.bincount(rows[:, G.LRF["STATUS"]].astype(int), minlength=6)[1:].tolist()
    conv = rows[rows[:, G.LRF["STATUS"]] == G.LRF_STATUS["CONVERGED"]]
    res = dict(case=case, members=M, lattice_rays=len(th), levels=len(LEVELS), stations=STATIONS, spec=SPEC, seeds=int(st[2]), rounds=int(st[0]), rays_per_round=3 * int(st[2]),
               ray_members=int(st[1]), status_counts=dict(zip(("converged", "iter_limit", "stalled", "lost", "singular"), status)),
               rounds_of_the_converged=np.bincount(conv[:, G.LRF["ITER"]].astype(int)).tolist() if len(conv) else [],
               worst_converged_miss_km=round(float(conv[:, G.LRF["MISS"]].max()), 5) if len(conv) else None,
               lattice_launch_event_ms=spread(lattice[1:]), level_stations_event_ms=spread(lists[1:]), refine_launches_event_ms=spread(launches[1:]),
               refine_own_kernels_event_ms=spread(kernels[1:]), refine_call_wall_ms=spread(wall[1:]))
    res["launch_ms_per_round"] = round(res["refine_launches_event_ms"]["median"] / max(1, res["rounds"]), 3)
    res["round_launch_share_of_lattice_launch"] = round(res["launch_ms_per_round"] / res["lattice_launch_event_ms"]["median"], 4)
    res["own_kernels_share_of_call"] = round(res["refine_own_kernels_event_ms"]["median"] / res["refine_call_wall_ms"]["median"], 5)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_refine_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_level_refine.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) with levels {LEVELS} km, {LVL_CAP} crossings kept; {STATIONS} stations on a ring of",
             f"# 1 degree around the source, dealt to the levels in turn; lists with ord_max {ORD_MAX}, cap {CAP}; refinement spec {SPEC}; library {G.build_id()}",
             "# lattice_launch_event_ms: one launch of the lattice (geoac_last_timing); refine_launches_event_ms: the sum of the same figure over a call's rounds (3 rays per seed,",
             "# through every member); refine_own_kernels_event_ms: HIP events around k_lrf_step of every round and k_lrf_rows; refine_call_wall_ms: host clock around the call + a stream sync;",
             f"# median / min / max of {a.reps} warm repetitions (lattice launch, lists, refinement) after one untimed one"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_level_refine: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
