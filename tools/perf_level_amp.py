"""Level amplitudes at the size of their use: the measured case of tools/perf_level_refine.py - the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2,
CalcAmp, ToyAtmo) launched with four levels (10 / 20 / 35 / 110 km), plain and from 8 sources, its level-station lists for 64 ring stations refined by
geoac_fan_level_refine - followed by geoac_fan_level_amp, which reads the refinement's final launch (its own two kernels and the medium probe kernel, no
launch), and by geoac_fan_level_amp_at for the same rows (the seeds' best angles, levels and branches), which costs one round's launch.  Per case, in
one process: the refinement call's launches and kernels beside level_amp()'s kernels and host wall clock, and level_amp_at()'s launch, kernels and wall
clock.  Median, min and max of --reps warm repetitions after one untimed one.  Every case is a child process of its own under a time limit; a child
that fails ends the run.
usage: perf_level_amp.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
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
from perf_level_refine import CASES, STATIONS, SPEC                              # noqa: E402


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
    R, A = G.LRF, G.LAMP
    t = {k: [] for k in ("refine_launches", "refine_kernels", "refine_wall", "amp_kernels", "amp_wall", "at_launch", "at_kernels", "at_wall")}
    for r in range(reps + 1):
        ctx.set_angles(th, ph)
        ctx.launch()
        ctx._chk(ctx.lib.geoac_fan_level_stations(ctx._h, ctypes.byref(lspec), len(sta), sta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), lv.ctypes.data_as(ctypes.c_void_p)))
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.geoac_fan_level_refine(ctx._h, ctypes.byref(rspec)))
        ctx._chk(ctx.lib.geoac_fan_sync(ctx._h))
        t["refine_wall"].append((time.perf_counter() - t0) * 1e3)
        ms = ctx.level_refine_timing()
        t["refine_launches"].append(ms["launch_ms"]); t["refine_kernels"].append(ms["kernel_ms"])
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.geoac_fan_level_amp(ctx._h))
        t["amp_wall"].append((time.perf_counter() - t0) * 1e3)
        ms = ctx.level_amp_timing()
        assert ms["launch_ms"] == 0.0
        t["amp_kernels"].append(ms["kernel_ms"])
        rows = ctx._level_amp_rows()[0]
        n, it = ctypes.c_int(0), ctypes.c_int(0)
        ctx._chk(ctx.lib.geoac_fan_level_refine_shape(ctx._h, ctypes.byref(n), ctypes.byref(it)))
        rr = np.empty((n.value, G.LRF_STRIDE))
        ctx._chk(ctx.lib.geoac_fan_level_refine_fetch(ctx._h, rr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        # the same rows through the primitive: every member integrates every seed's three rays, a seed's own member's row is the one compared
        t0 = time.perf_counter()
        at = ctx.level_amp_at(rr[:, R["THETA"]].copy(), rr[:, R["PHI"]].copy(), lv[rr[:, R["STATION"]].astype(int)], rr[:, R["LEG"]].astype(int), rr[:, R["DIR"]].astype(int),
                              rr[:, R["ORD"]].astype(int), probe_deg=SPEC["probe_deg"])
        t["at_wall"].append((time.perf_counter() - t0) * 1e3)
        ms = ctx.level_amp_timing()
        t["at_launch"].append(ms["launch_ms"]); t["at_kernels"].append(ms["kernel_ms"])
    conv = rr[:, R["STATUS"]] == G.LRF_STATUS["CONVERGED"]
    own = at[rr[:, R["MEMBER"]].astype(int), np.arange(len(rr))]
    cols = [k for k in range(G.LAMP_STRIDE) if k != A["INDEX"]]
    same = bool(np.array_equal(rows[conv][:, cols].view(np.uint64), own[conv][:, cols].view(np.uint64)))
    st = np.bincount(rows[:, A["STATUS"]].astype(int), minlength=6)[1:].tolist()
    ok = rows[:, A["STATUS"]] == G.LAMP_STATUS["OK"]
    M = 8 if case == "sources8" else 1
    res = dict(case=case, members=M, lattice_rays=len(th), levels=len(LEVELS), stations=STATIONS, spec=SPEC, seeds=int(len(rr)), converged=int(conv.sum()),
               level_amp_status_counts=dict(zip(("ok", "absent", "no_probe", "singular", "skipped"), st)),
               amp_db_range=[round(float(20.0 * np.log10(rows[ok, A["AMP"]].min())), 2), round(float(20.0 * np.log10(rows[ok, A["AMP"]].max())), 2)] if ok.any() else None,
               converged_rows_equal_level_amp_at_bits=same,
               refine_launches_event_ms=spread(t["refine_launches"][1:]), refine_own_kernels_event_ms=spread(t["refine_kernels"][1:]), refine_call_wall_ms=spread(t["refine_wall"][1:]),
               level_amp_kernels_event_ms=spread(t["amp_kernels"][1:]), level_amp_call_wall_ms=spread(t["amp_wall"][1:]),
               level_amp_at_launch_event_ms=spread(t["at_launch"][1:]), level_amp_at_kernels_event_ms=spread(t["at_kernels"][1:]), level_amp_at_call_wall_ms=spread(t["at_wall"][1:]))
    res["level_amp_share_of_refine_call"] = round(res["level_amp_call_wall_ms"]["median"] / res["refine_call_wall_ms"]["median"], 5)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_amp_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_level_amp.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) with levels {LEVELS} km, {LVL_CAP} crossings kept; {STATIONS} stations on a ring of",
             f"# 1 degree around the source, dealt to the levels in turn; lists with ord_max {ORD_MAX}, cap {CAP}; refinement spec {SPEC}; library {G.build_id()}",
             "# refine_*: the geoac_fan_level_refine call before (tools/perf_level_refine.py's figures); level_amp_kernels_event_ms: HIP events around k_lamp_gather, the medium probe kernel and",
             "# k_lamp_rows of geoac_fan_level_amp (no launch); level_amp_call_wall_ms: host clock around that call (it ends with a stream sync); level_amp_at_*: geoac_fan_level_amp_at for the same",
             "# rows - one fan of 3 rays per seed through every member (launch), the same three kernels, host clock around the call with its fetch;",
             f"# median / min / max of {a.reps} warm repetitions (lattice launch, lists, refinement, level_amp, level_amp_at) after one untimed one"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_level_amp: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
