"""Arrival maps against what they replace: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) binned on a 256 x 512 lat/lon grid,
plain, from 8 sources and at 16 frequencies.  Per case, in one process, after the launch: `map` - geoac_fan_map by HIP events and by host wall clock
(the call returns when the kernels are enqueued; the wall time includes a stream sync), `map_fetch` - all layers, outside and detect to the host;
against the parent interface: `fetch` - fetch() of the records (plus fetch_atten() with a frequency set), and `host_binning` - tests/map_reference.py
on the fetched tables, reported apart.  Median, min and max of --reps warm rounds after one untimed round.  Every case is a child process of its
own under a time limit; a child that fails ends the run.
usage: perf_map.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME --once]"""
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

GRID = dict(origin=(12.0, -20.0), step=(36.0 / 256, 40.0 / 512), n=(256, 512), detect_db=-70.0)
CASES = ("plain", "sources8", "freqs16")


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def step(case, reps, once):
    import geoac_amd as G
    import harness as H
    import map_reference as MR
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    if case == "sources8":
        ctx.set_sources(np.array([[0.0, 28.0 + 0.5 * s, -2.0 + 0.5 * s] for s in range(8)]))
    if case == "freqs16":
        ctx.set_frequencies([float(f"{v:.4g}") for v in np.logspace(np.log10(0.05), np.log10(5.0), 16)])
    ctx.set_angles(th, ph)
    ctx.launch()
    launch_ms = ctx.timing()["ms_total"]
    if once:                                                           # one map call, for a kernel trace
        ctx.map(**GRID)
        ctx.close()
        return dict(case=case)
    ev, wall, mfetch, fetch, host = [], [], [], [], []
    spec = G.map_spec(**GRID)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.geoac_fan_map(ctx._h, ctypes.byref(spec)))
        ctx._chk(ctx.lib.geoac_fan_sync(ctx._h))
        t1 = time.perf_counter()
        out = ctx.map(spec)                                            # (binning again + the fetch of every layer)
        t2 = time.perf_counter()
        ev.append(ctx.map_timing()); wall.append((t1 - t0) * 1e3); mfetch.append((t2 - t1) * 1e3 - ev[-1])
        t0 = time.perf_counter()
        rec, _ = ctx.fetch()
        att = ctx.fetch_atten() if case == "freqs16" else None
        fetch.append((time.perf_counter() - t0) * 1e3)
    rec = rec.reshape((-1,) + rec.shape[-3:])
    level = ctx.fetch_level()
    if att is None:
        att = rec[0, :, :, G.REC["ATTEN"]][None]
    for r in range(2):
        t0 = time.perf_counter()
        ref = MR.reference_map(G.EQ_GLOBAL, rec, MR.level_numpy(rec, att, 1), MR.spec(**GRID))
        host.append((time.perf_counter() - t0) * 1e3)
    ref = MR.reference_map(G.EQ_GLOBAL, rec, level, MR.spec(**GRID))
    MR.assert_maps_equal(out, ref)
    ctx.close()
    res = dict(case=case, members=int(rec.shape[0]), freqs=int(level.shape[1]), records=int(rec.shape[0] * rec.shape[1] * rec.shape[2]),
               record_MB=round(rec.nbytes / 1e6, 1), layer_MB=round(sum(v.nbytes for v in out.values()) / 1e6, 1),
               arrivals=ref["n_pass"], inside=int(out["count"].sum()), launch_event_ms=round(launch_ms, 2),
               map_event_ms=spread(ev[1:]), map_wall_ms=spread(wall[1:]), map_fetch_ms=spread(mfetch[1:]),
               map_plus_fetch_ms=spread([a + b for a, b in zip(wall[1:], mfetch[1:])]),
               fetch_records_ms=spread(fetch[1:]), host_binning_ms=spread(host), equals_reference=True)
    res["map_plus_fetch_shorter_than_record_fetch"] = bool(res["map_plus_fetch_ms"]["median"] < res["fetch_records_ms"]["median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_perf.txt"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--case")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps, a.once)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_map.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) binned on a 256 x 512 lat/lon grid; library {G.build_id()}",
             "# map_event_ms: HIP events around the kernels of geoac_fan_map; map_wall_ms: the call + a stream sync; map_fetch_ms: all layers, outside and detect to the host;",
             "# fetch_records_ms: fetch() (+ fetch_atten() with a frequency set), what a host binning has to move first; host_binning_ms: tests/map_reference.py on those tables.",
             f"# median / min / max of {a.reps} warm rounds after one untimed round (host_binning: 2 rounds); every map was checked bit for bit against the reference"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_map: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
