"""Grid ensembles against sequential plain-context passes, both grid sets on the 5 x 5 x 1400 grid of config 4 (tests/golden/rngdep_grid_1400.npz; the spherical set
holds the same columns on the latitude / longitude nodes of tests/rngdep_data.py): a fan of 60 azimuths x 40 inclinations (2 400 rays, bounces 1, CalcAmp) through
K = 1, 2, 4, 8 members - member 0 the grid itself, the others with the winds scaled by 0.7 - 1.3 and T shifted by up to +-4 K.  Per K: one geoac_fan_launch through the
K members (one lane per ray) against K launches of plain contexts one after the other in the same process, each under the plan's own choice of kernel (small plain fans get
the multi-lane kernels).  HIP-event time of the launches; median of the warm rounds with min - max.
usage: perf_grid_ensemble.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geoac_amd as G  # noqa: E402
import rngdep_data as RD  # noqa: E402

WIND = [1.0, 1.3, 0.7, 1.2, 0.8, 1.15, 0.85, 1.1]
DT = [0.0, 4.0, -4.0, 2.5, -2.5, 3.0, -3.0, 1.0]
KS = (1, 2, 4, 8)


def write_global_1400(dirpath):
    """the 1400-level columns as a spherical grid: g<n>.met + latitude / longitude node files"""
    os.makedirs(dirpath, exist_ok=True)
    z, T, u, v, rho, p = RD.load_grid_columns(1)
    prefix = os.path.join(dirpath, "g")
    for i in range(len(RD.LAT_NODES)):
        for j in range(len(RD.LON_NODES)):
            with open(f"{prefix}{i * len(RD.LON_NODES) + j}.met", "w") as fh:
                for k in range(len(z)):
                    fh.write(f"{z[k]:.10g} {T[i, j, k]:.12g} {u[i, j, k]:.12g} {v[i, j, k]:.12g} {rho[i, j, k]:.12g} {p[k]:.10g}\n")
    la, lo = os.path.join(dirpath, "loc_lat.dat"), os.path.join(dirpath, "loc_lon.dat")
    with open(la, "w") as fh:
        fh.write("".join(f"{x:.10g}\n" for x in RD.LAT_NODES))
    with open(lo, "w") as fh:
        fh.write("".join(f"{y:.10g}\n" for y in RD.LON_NODES))
    return prefix, la, lo


def stats(v):
    return dict(median=round(float(np.median(v)), 2), min=round(float(np.min(v)), 2), max=round(float(np.max(v)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    th, ph = G.fan_enumerate(theta_min=1.0, theta_max=40.0, theta_step=1.0, phi_min=-180.0, phi_max=-180.0 + 59 * 6.0, phi_step=6.0)
    lines = []
    for name, eq, src in (("GeoAc3D.RngDep", G.EQ_3D_RNGDEP, (0.0, 0.0, 0.0)), ("GeoAcGlobal.RngDep", G.EQ_GLOBAL_RNGDEP, (0.0, 31.0, 0.0))):
        tmp = os.path.join(tempfile.gettempdir(), "perf_grid_ens_" + name)
        files = write_global_1400(tmp) if eq == G.EQ_GLOBAL_RNGDEP else RD.write_grid(tmp, short_paths=False, thin=1)
        params = dict(bounces=1, calc_amp=1, mode=0, src=src)
        plain = []
        for m in range(max(KS)):
            ctx = G.FanContext(eq, device=0)
            if m == 0:
                g = ctx.load_grid(*files)
            else:
                ctx.upload_atmo_3d(g["x"], g["y"], g["z"], g["T"] + DT[m], g["u"] * WIND[m], g["v"] * WIND[m], g["rho"])
            ctx.set_params(**params)
            ctx.set_angles(th, ph)
            ctx.launch()                                          # warm-up (buffers)
            plain.append(ctx)
        seq = {K: [] for K in KS}
        for _ in range(args.reps):
            ms = []
            for ctx in plain:                                     # K passes one after the other: the first K of these
                ctx.launch()
                ms.append(ctx.timing()["ms_total"])
            for K in KS:
                seq[K].append(sum(ms[:K]))
        steps1 = [ctx.total_steps() for ctx in plain]
        print(f"# {name}: {len(th)} rays, plain passes done, ray-steps per member {steps1}", flush=True)
        for ctx in plain:
            ctx.close()
        for K in KS:
            ctx = G.FanContext(eq, device=0)
            ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([f(m) for m in range(K)]) for f in
                                        (lambda m: g["T"] + DT[m], lambda m: g["u"] * WIND[m], lambda m: g["v"] * WIND[m], lambda m: g["rho"])])
            ctx.set_params(**params)
            ctx.set_angles(th, ph)
            ctx.launch()
            ens = []
            for _ in range(args.reps):
                ctx.launch()
                ens.append(ctx.timing()["ms_total"])
            steps = ctx.total_steps()
            ctx.close()
            assert steps == sum(steps1[:K]), (name, K, steps, steps1)
            e, s = stats(ens), stats(seq[K])
            row = dict(set=name, K=K, rays=len(th) * K, ray_steps=steps, ensemble_ms=e, sequential_ms=s, speedup_of_medians=round(s["median"] / e["median"], 3),
                       ensemble_ray_steps_per_s=float(f"{steps / e['median'] * 1e3:.4g}"), sequential_ray_steps_per_s=float(f"{steps / s['median'] * 1e3:.4g}"))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    hdr = (f"# tools/perf_grid_ensemble.py: 5 x 5 x 1400 grid, fan of 60 azimuths x 40 inclinations (2 400 rays), bounces 1, CalcAmp; HIP-event ms of the launches, median (min - max) of "
           f"{args.reps} warm rounds after one warm-up each; library {G.build_id()}\n"
           f"# ensemble_ms: one launch through K members (one lane per ray); sequential_ms: K launches of plain contexts one after the other, each under the plan's own kernel\n")
    if args.out:
        with open(args.out, "w") as f:
            f.write(hdr + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
