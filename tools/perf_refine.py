"""Station refinement against what it replaces: the 64 stations of the 2.5-degree ring around (30 N, 0 E) on the 0.5 x 1 degree Global lattice over
the whole azimuth circle (GeoAcGlobal, ToyAtmo, one bounce, CalcAmp), run as a plain context, an ensemble of 8, from 8 sources and at 16
frequencies.  Per case, in one process: the lattice launch and geoac_fan_stations once, then per round of --reps + 1 (the first untimed) lattice
launch, stations and `refine` - geoac_fan_refine by host wall clock, with its own split (HIP-event time of its launches, of its kernels), rounds
used, ray-members integrated against used (the M-fold discard).  Baseline: today's only route, geoac_eig_direct seeded with the same estimates
(INTEGRATION 3g), on one plain context per member, one after the other, one call per leg (the call takes one bounce count).  Every case is a child
process of its own under a time limit; a child that fails ends the run.
usage: perf_refine.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("plain", "ensemble8", "sources8", "freqs16")
CAP = 8
SPEC = dict(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2)


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def step(case, reps):
    import geoac_amd as G
    import harness as H
    from parity import ring_receivers
    from test_gpu_ensemble import _device_arrays, _raw_members
    eq = G.EQ_GLOBAL
    S, R = G.STA, G.RFN
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt, nph = 90, 360
    sta = ring_receivers(n=64, lat0=30.0, lon0=0.0, radius_deg=2.5)
    raw = np.loadtxt(H.TOYATMO)
    toy = _device_arrays(eq, *[raw[:, k] for k in range(5)])
    profs = [toy]
    srcs = np.array([[0.0, 30.0, 0.0]])
    freqs = [0.1]
    if case == "ensemble8":
        w = np.linspace(0.8, 1.2, 8)
        profs = [_device_arrays(eq, *r) for r in _raw_members(wind=tuple(w), dT=tuple(np.linspace(-3.0, 3.0, 8)))]
    if case == "sources8":
        srcs = np.array([[0.0, 30.0 + 0.05 * s, 0.05 * s] for s in range(8)])
    if case == "freqs16":
        freqs = [float(f"{v:.4g}") for v in np.logspace(np.log10(0.05), np.log10(5.0), 16)]
    ctx = G.FanContext(eq, device=0)
    if len(profs) > 1:
        ctx.upload_atmo_1d_ensemble(profs[0][0], *[np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)])
    else:
        ctx.upload_atmo_1d(*toy)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(srcs[0]))
    if len(srcs) > 1:
        ctx.set_sources(srcs)
    if len(freqs) > 1:
        ctx.set_frequencies(freqs)
    spec = G.station_spec(nt, nph, phi_periodic=True, cap=CAP)
    wall, launch_ms, kernel_ms, lattice_ms = [], [], [], []
    for r in range(reps + 1):
        ctx.set_angles(th, ph)
        ctx.launch()
        lattice_ms.append(ctx.timing()["ms_total"])
        hits, srows, _ = ctx.stations(spec, sta)
        t0 = time.perf_counter()
        rows, level, stats = ctx.refine(**SPEC)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = ctx.refine_timing()
        launch_ms.append(t["launch_ms"]); kernel_ms.append(t["kernel_ms"])
    ctx.close()
    M = hits.shape[0]
    res = dict(case=case, members=M, freqs=len(freqs), lattice_rays=len(th), lattice_launch_ms=spread(lattice_ms[1:]), seeds=stats["seeds"], converged=stats["converged"],
               stalled_or_limit=stats["stalled_or_limit"], lost_or_singular=stats["lost_or_singular"], rounds=stats["launches"], ray_members_integrated=stats["ray_members"],
               ray_members_used=stats["launches"] * stats["seeds"], refine_wall_ms=spread(wall[1:]), refine_launches_event_ms=spread(launch_ms[1:]),
               refine_kernels_event_ms=spread(kernel_ms[1:]), ms_per_round=round(float(np.median(wall[1:])) / max(1, stats["launches"]), 3))
    # baseline: geoac_eig_direct seeded with the same estimates, one plain context per member (the frequency set: one context, its first frequency -
    # the other 15 levels would need 15 more), one call per leg
    base, found = [], 0
    for r in range(min(reps, 2) + 1):
        t0 = time.perf_counter()
        found = 0
        for m in range(M):
            c2 = G.FanContext(eq, device=0)
            c2.upload_atmo_1d(*profs[m % len(profs)])
            c2.set_params(calc_amp=1, src=tuple(srcs[m // len(profs)]), freq=freqs[0])
            est = [(s, k) for s in range(len(sta)) for k in range(min(int(hits[m, s]), CAP))]
            for leg in sorted({int(srows[m, s, k, S["LEG"]]) for s, k in est}):
                sel = [(s, k) for s, k in est if int(srows[m, s, k, S["LEG"]]) == leg]
                out = c2.eig_direct(sta[[s for s, _ in sel]], np.array([srows[m, s, k, S["THETA"]] for s, k in sel]), np.array([srows[m, s, k, S["PHI"]] for s, k in sel]),
                                    bounces=leg)
                found += len(out["eig"])
            c2.close()
        base.append((time.perf_counter() - t0) * 1e3)
    res["eig_direct_wall_ms"] = spread(base[1:])
    res["eig_direct_eigenrays"] = found
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_refine.py: 64 stations of the 2.5-degree ring on the 0.5 x 1 degree Global lattice (360 x 90 rays, one bounce, CalcAmp, ToyAtmo), cap {CAP}, spec {SPEC}; library {G.build_id()}",
             "# refine_wall_ms: geoac_fan_refine and the fetch of its rows by host wall clock; refine_launches_event_ms / refine_kernels_event_ms: its own split (HIP events);",
             "# ray_members_integrated against ray_members_used: the M-fold discard; eig_direct_wall_ms: geoac_eig_direct with the same estimates, one plain context per member, one after the other",
             f"# (context set-up included; a frequency set: its first frequency only); median / min / max of {a.reps} warm rounds after one untimed round (eig_direct: 2 after one)"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_refine: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
