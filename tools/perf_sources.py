"""Source sets against sequential single-source passes: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp, ToyAtmo) from n_src = 1, 2, 4, 8
sources on the meridian through the default source (0 km, 30 N, 0 E), 5 degrees apart (30, 35, 25, 40, 20, 45, 15, 50 N).  Per n_src, in one
process: ms of each single-source pass (a context of its own, the source in its parameters), then ms of the one launch over the set (HIP-event time
of the launch, median of --reps after one warm-up).  Every n_src is a child process of its own under a time limit; a child that fails ends the run.
usage: perf_sources.py [--reps N] [--out FILE] [--timeout SECONDS] [--trace N_SRC]      (--trace: one more launch of that set with per-epoch live counts on stderr)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LATS = [30.0, 35.0, 25.0, 40.0, 20.0, 45.0, 15.0, 50.0]


def pass_ms(ctx, th, ph, reps):
    ctx.set_angles(th, ph)
    ctx.launch()                                              # warm-up (tables, buffers)
    ms = []
    for _ in range(reps):
        ctx.launch()
        ms.append(ctx.timing()["ms_total"])
    return float(np.median(ms)), ctx.total_steps()


def step(n_src, reps, trace):
    import geoac_amd as G
    import harness as H
    src = np.array([[0.0, lat, 0.0] for lat in LATS[:n_src]])
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    single = []
    for s in src:
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=2, calc_amp=1, src=tuple(s))
        single.append(pass_ms(ctx, th, ph, reps))
        ctx.close()
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_sources(src)
    ms, steps = pass_ms(ctx, th, ph, reps)
    epochs = ctx.timing()["epochs"]
    ctx.close()
    seq_ms = sum(s[0] for s in single); seq_steps = sum(s[1] for s in single)
    assert steps == seq_steps, (n_src, steps, seq_steps)
    row = dict(n_src=n_src, rays=len(th) * n_src, ray_steps=steps, epochs=epochs, one_launch_ms=round(ms, 2), sequential_ms=round(seq_ms, 2),
               single_pass_ms=[round(s[0], 2) for s in single],
               one_launch_ray_steps_per_s=float(f"{steps / ms * 1e3:.4g}"), sequential_ray_steps_per_s=float(f"{seq_steps / seq_ms * 1e3:.4g}"),
               speedup=round(seq_ms / ms, 3), library=G.build_id())
    print(json.dumps(row), flush=True)
    if trace:
        ctx = G.FanContext(G.EQ_GLOBAL, device=0, options={"TRACE_EPOCHS": "1"})
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=2, calc_amp=1)
        ctx.set_sources(src)
        ctx.set_angles(th, ph)
        ctx.launch()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.trace == args.step)
        return
    rows = []
    for n_src in (1, 2, 4, 8):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", str(n_src), "--reps", str(args.reps), "--trace", str(args.trace)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"n_src = {n_src}: exit status {r.returncode}; nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(r.stdout.strip(), flush=True)
    lib = rows[0]["library"]
    hdr = (f"# tools/perf_sources.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp, ToyAtmo) from n_src sources at 0 km, 0 E and "
           f"{', '.join(f'{lat:g}' for lat in LATS)} N; median of {args.reps} passes after one warm-up; library {lib}\n"
           f"# per n_src, in one process: the single-source passes (single_pass_ms, one context each, in the order of the sources), then one launch over the set\n")
    if args.out:
        with open(args.out, "w") as f:
            f.write(hdr + "\n".join(json.dumps({k: v for k, v in r.items() if k != "library"}) for r in rows) + "\n")


if __name__ == "__main__":
    main()
