"""Station arrivals against what they replace: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo), plain, from 8 sources
and at 16 frequencies, searched for R = 64 / 1 024 / 16 384 stations on rings of 1 .. 8 degrees around the source.  Per case, in one process,
after the launch: `stations` - geoac_fan_stations by HIP events and by host wall clock (the call + a stream sync), `lists_fetch` - hits, rows and
level to the host; against the parent interface: `fetch` - fetch() of the records (plus fetch_atten() with a frequency set) and `host_search` -
tests/station_reference.py on the fetched tables (R = 64, and 1 024 for a single member; one round), and, for the plain launch and R = 64, geoac_eig_search on the same
ring.  Median, min and max of --reps warm rounds after one untimed round.  Every case is a child process of its own under a time limit; a child
that fails ends the run.
usage: perf_stations.py [--reps N] [--out FILE] [--timeout SECONDS] [--case NAME --once R]"""
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

CASES = ("plain", "sources8", "freqs16")
STATIONS = (64, 1024, 16384)
CAP = 16


def spread(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(min(ms)), 3), max=round(float(max(ms)), 3))


def rings(n, lat0=30.0, lon0=0.0):
    """n stations on rings of 64 around the source, radii from 1 to 8 degrees of arc (R = 64: the 2.5-degree ring of config 5)"""
    k = np.arange(n)
    az = (k % 64) * (2.0 * np.pi / 64)
    rad = np.full(n, 2.5) if n <= 64 else 1.0 + 7.0 * (k // 64) / max(1, n // 64 - 1)
    return np.stack([lat0 + rad * np.cos(az), lon0 + rad * np.sin(az) / np.cos(np.radians(lat0))], axis=1)


def step(case, reps, once):
    import geoac_amd as G
    import harness as H
    import station_reference as SR
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    nt, nph = 90, 360
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
    spec = G.station_spec(nt, nph, phi_periodic=True, cap=CAP)
    if once:                                                           # one call, for a kernel trace
        ctx.stations(spec, rings(once))
        ctx.close()
        return dict(case=case)
    fetch = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        rec, _ = ctx.fetch()
        att = ctx.fetch_atten() if case == "freqs16" else None
        fetch.append((time.perf_counter() - t0) * 1e3)
    rec = rec.reshape((-1,) + rec.shape[-3:])
    level = ctx.fetch_level()
    res = dict(case=case, members=int(rec.shape[0]), freqs=int(level.shape[1]), rays=int(rec.shape[1]), legs=int(rec.shape[2]), record_MB=round(rec.nbytes / 1e6, 1),
               launch_event_ms=round(launch_ms, 2), fetch_records_ms=spread(fetch[1:]), by_stations={})
    for R in STATIONS:
        sta = rings(R)
        ev, wall, lfetch = [], [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.geoac_fan_stations(ctx._h, ctypes.byref(spec), len(sta), sta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            ctx._chk(ctx.lib.geoac_fan_sync(ctx._h))
            t1 = time.perf_counter()
            out = ctx.stations(spec, sta)                              # (the search again + the fetch of the lists)
            t2 = time.perf_counter()
            ev.append(ctx.stations_timing()); wall.append((t1 - t0) * 1e3); lfetch.append((t2 - t1) * 1e3 - ev[-1])
        one = dict(stations=R, list_MB=round(sum(v.nbytes for v in out) / 1e6, 2), hits=int(out[0].sum()), stations_with_hits=int((out[0] > 0).any(axis=0).sum()),
                   most_hits=int(out[0].max()), stations_event_ms=spread(ev[1:]), stations_wall_ms=spread(wall[1:]), lists_fetch_ms=spread(lfetch[1:]),
                   stations_plus_fetch_ms=spread([a + b for a, b in zip(wall[1:], lfetch[1:])]))
        one["stations_plus_fetch_shorter_than_record_fetch"] = bool(one["stations_plus_fetch_ms"]["median"] < res["fetch_records_ms"]["median"])
        one["event_share_of_launch"] = round(one["stations_event_ms"]["median"] / launch_ms, 4)
        if R <= 64 or (R <= 1024 and rec.shape[0] == 1):
            t0 = time.perf_counter()
            ref = SR.reference_stations(G.EQ_GLOBAL, rec, th, ph, level, SR.spec(nt, nph, phi_periodic=True, cap=CAP), sta, block=8)
            one["host_search_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            SR.assert_lists_equal(out, ref)
            one["equals_reference"] = True
        res["by_stations"][str(R)] = one
    ctx.close()
    if case == "plain":                                                # the search the estimates would seed, on the same 64-ring
        c2 = G.FanContext(G.EQ_GLOBAL, device=0)
        c2.load_met(H.TOYATMO)
        c2.set_params(src=(0.0, 30.0, 0.0))
        eig = []
        for r in range(3):
            t0 = time.perf_counter()
            out = c2.eig_search(rings(64), bnc_min=0, bnc_max=2)
            eig.append((time.perf_counter() - t0) * 1e3)
        res["eig_search_64_ring_ms"] = spread(eig[1:])
        res["eig_search_64_ring_eigenrays"] = int(len(out["eig"]))
        c2.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stations_perf.txt"))
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--case")
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(step(a.case, a.reps, a.once)), flush=True)
        return
    import geoac_amd as G
    lines = [f"# tools/perf_stations.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo), stations on rings of 1 .. 8 degrees around the source, cap {CAP}; library {G.build_id()}",
             "# stations_event_ms: HIP events around geoac_fan_stations; stations_wall_ms: the call + a stream sync; lists_fetch_ms: hits, rows and level to the host;",
             "# fetch_records_ms: fetch() (+ fetch_atten() with a frequency set), what a host search has to move first; host_search_ms: tests/station_reference.py on those tables (one round);",
             f"# median / min / max of {a.reps} warm rounds after one untimed round; every list that has a host_search_ms was checked bit for bit against the reference"]
    for case in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"perf_stations: case {case} failed (exit {p.returncode})")
        print(got[0][7:], flush=True)
        lines.append(got[0][7:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
