"""Frequency sets against sequential single-frequency passes: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) at F = 1, 2, 4, 8, 16
frequencies spaced logarithmically over 0.05 - 5 Hz.  Per F, in one process: `sequential` - one context, per frequency set_params(freq=f) and a
launch, which is what a band costs without the set (the absorption-table rebuild of every pass included: the frequency changes each time) - then
`one_launch` - set_frequencies(freqs) and one launch.  Both are host wall-clock times around the launch calls (the launch returns when the fan has
finished), warm: one untimed round first, then --reps rounds; median, min and max are reported, and the HIP-event time of the one launch beside them.
Every F is a child process of its own under a time limit; a child that fails ends the run.
usage: perf_freqs.py [--reps N] [--out FILE] [--timeout SECONDS]"""
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


def band(F):
    return [0.1] if F == 1 else [float(f"{v:.4g}") for v in np.logspace(np.log10(0.05), np.log10(5.0), F)]


def spread(ms):
    return dict(median=round(float(np.median(ms)), 2), min=round(float(min(ms)), 2), max=round(float(max(ms)), 2))


def step(F, reps):
    import geoac_amd as G
    import harness as H
    freqs = band(F)
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    # sequential passes on one context
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_angles(th, ph)
    seq, col = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        for f in freqs:
            ctx.set_params(freq=f)
            ctx.launch()
        seq.append((time.perf_counter() - t0) * 1e3)
    steps1 = ctx.total_steps()
    for f in freqs:                                               # (untimed: the columns the set has to reproduce)
        ctx.set_params(freq=f)
        ctx.launch()
        col.append(ctx.fetch()[0][:, :, G.REC["ATTEN"]].copy())
    ctx.close()
    # one launch over the set
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_frequencies(freqs)
    ctx.set_angles(th, ph)
    one, ev, post = [], [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ctx.launch()
        one.append((time.perf_counter() - t0) * 1e3)
        t = ctx.timing()
        ev.append(t["ms_total"]); post.append(t["ms_post"])
    att = ctx.fetch_atten()
    steps, epochs, info = ctx.total_steps(), ctx.timing()["epochs"], ctx.abs_table_info()
    ctx.close()
    assert steps == steps1
    same = all(np.array_equal(att[f].view(np.uint64), col[f].view(np.uint64)) for f in range(F))
    assert same, "the set's attenuation differs from the sequential passes"
    s, o = spread(seq[1:]), spread(one[1:])
    row = dict(F=F, freqs=freqs, ray_steps=steps, epochs=epochs, sequential_ms=s, one_launch_ms=o, one_launch_event_ms=spread(ev[1:]), one_launch_post_ms=spread(post[1:]),
               speedup=round(s["median"] / o["median"], 3), per_frequency_ms=round(o["median"] / F, 2), table_entries=info["entries"], bit_identical=same, library=G.build_id())
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return
    rows = []
    for F in (1, 2, 4, 8, 16):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", str(F), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"F = {F}: exit status {r.returncode}; nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(r.stdout.strip(), flush=True)
    lib = rows[0]["library"]
    hdr = (f"# tools/perf_freqs.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) at F frequencies, logarithmically spaced over 0.05 - 5 Hz (F = 1: 0.1 Hz); "
           f"library {lib}\n"
           f"# sequential_ms: F passes with set_params(freq=f) between them, table rebuild included; one_launch_ms: set_frequencies + one launch; host wall-clock ms around the launch\n"
           f"# calls, median / min / max of {args.reps} warm rounds after one untimed round; one_launch_event_ms, one_launch_post_ms: HIP-event times of the launch and of its post-pass stream\n")
    if args.out:
        with open(args.out, "w") as f:
            f.write(hdr + "\n".join(json.dumps({k: v for k, v in r.items() if k != "library"}) for r in rows) + "\n")


if __name__ == "__main__":
    main()
