"""Ensemble fans against sequential single-profile passes: the metric fan (GeoAcGlobal, 360 x 90 rays, bounces 2, CalcAmp) through K = 1, 2, 4, 8
profiles - member 0 ToyAtmo, the others ToyAtmo with the winds scaled by 0.6 - 1.4 and T shifted by up to +-5 K.  Per K: ms per ensemble pass (one
geoac_fan_launch, HIP-event time of the launch), ms of the K single-context passes one after the other, and ray-steps/s of both.
usage: perf_ensemble.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geoac_amd as G  # noqa: E402
import harness as H  # noqa: E402

WIND = [1.0, 1.4, 0.6, 1.2, 0.8, 1.3, 0.7, 1.1]
DT = [0.0, 5.0, -5.0, 2.5, -2.5, 4.0, -4.0, 1.0]


def members(a, K):
    return [(a["T"] + DT[m], a["u"] * WIND[m], a["v"] * WIND[m], a["rho"]) for m in range(K)]


def pass_ms(ctx, th, ph, reps):
    ctx.set_angles(th, ph)
    ctx.launch()                                              # warm-up (tables, buffers)
    ms = []
    for _ in range(reps):
        ctx.launch()
        ms.append(ctx.timing()["ms_total"])
    return float(np.median(ms)), ctx.total_steps()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = G.met_load(H.TOYATMO, G.EQ_GLOBAL)
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    single = []
    for m, (T, u, v, rho) in enumerate(members(a, 8)):
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        ctx.upload_atmo_1d(a["x"], T, u, v, rho)
        ctx.set_params(bounces=2, calc_amp=1)
        single.append(pass_ms(ctx, th, ph, args.reps))
        ctx.close()
    lines = []
    for K in (1, 2, 4, 8):
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        mem = members(a, K)
        ctx.upload_atmo_1d_ensemble(a["x"], *[np.stack([p[i] for p in mem]) for i in range(4)])
        ctx.set_params(bounces=2, calc_amp=1)
        ms, steps = pass_ms(ctx, th, ph, args.reps)
        ctx.close()
        seq_ms = sum(s[0] for s in single[:K]); seq_steps = sum(s[1] for s in single[:K])
        assert steps == seq_steps, (K, steps, seq_steps)
        row = dict(K=K, rays=len(th) * K, ray_steps=steps, ensemble_ms=round(ms, 2), sequential_ms=round(seq_ms, 2),
                   ensemble_ray_steps_per_s=float(f"{steps / ms * 1e3:.4g}"), sequential_ray_steps_per_s=float(f"{seq_steps / seq_ms * 1e3:.4g}"),
                   speedup=round(seq_ms / ms, 3))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    hdr = (f"# tools/perf_ensemble.py: metric fan (GeoAcGlobal 360 x 90, bounces 2, CalcAmp), median of {args.reps} passes after one warm-up; "
           f"library {G.build_id()}\n# single-profile passes, ms: " + ", ".join(f"{s[0]:.2f}" for s in single) + "\n")
    if args.out:
        with open(args.out, "w") as f:
            f.write(hdr + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
