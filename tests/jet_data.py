"""Deterministic jet atmosphere for the stratified sets (2D, 3D, Global): tests/golden/JetAtmo.met, in the SECOND profile format `zuvwTdp`
(z, u, v, w, T, rho, p).  ToyAtmo's T, rho, p on 900 irregular nodes (spacing 0.2 .. 1.8 of the mean, every 20th segment 3 .. 10 m: shorter than an
RK4 step); u = ToyAtmo's u + an 85 m/s stratospheric jet at 56 km + 30 m/s at 11 km (-50 .. 38 m/s in all); v = 40 m/s at 47 km - 22 m/s at 12 km + 15 m/s at 105 km: a
meridional wind of tens of m/s that changes sign, and wind AT an elevated source (12 km).  The w column is not zero: no stratified set reads it, and a
parser that stored it anywhere would show.  The committed file is the data; `python tests/jet_data.py` rewrites it (same bytes wherever numpy's exp
rounds the same way), write_twin() writes the committed numbers in `zTuvdp` column order."""
import os

import numpy as np

import harness as H

JET = os.path.join(H.GOLDEN_DIR, "JetAtmo.met")
FMT = "zuvwTdp"
N_ROWS = 900
SEED = 5611
SRC_Z = 12.0                  # the elevated source of the fixtures: inside the tropospheric jet (u = 30, v = -22 m/s there)


def _bump(z, centre, width):
    return np.exp(-((z - centre) / width) ** 2)


def columns(n=N_ROWS, seed=SEED):
    """z, u, v, w, T, rho, p (raw .met units: km, m/s, K, g/cm^3, mbar)"""
    raw = np.loadtxt(H.TOYATMO)
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.2, 1.8, n - 1)
    h[rng.integers(0, n - 1, n // 20)] = 0.02                  # 3 .. 10 m segments
    z = np.concatenate([[0.0], np.cumsum(h)])
    z *= raw[-1, 0] / z[-1]
    z = np.round(z, 6)                                          # (what the file holds: the nodes are exact decimals)
    T, u0, rho, p = (np.interp(z, raw[:, 0], raw[:, c]) for c in (1, 2, 4, 5))
    u = u0 + 85.0 * _bump(z, 56.0, 8.0) + 30.0 * _bump(z, 11.0, 3.0)
    v = 40.0 * _bump(z, 47.0, 9.0) - 22.0 * _bump(z, 12.0, 3.5) + 15.0 * _bump(z, 105.0, 12.0)
    w = 0.05 + 0.3 * np.sin(z / 7.0)
    return z, u, v, w, T, rho, p


def write_met(path=JET):
    cols = columns()
    with open(path, "w") as fh:
        for row in zip(*cols):
            fh.write(" ".join([f"{row[0]:.10g}"] + [f"{x:.12g}" for x in row[1:]]) + "\n")
    return path


def _tokens():
    return [line.split() for line in open(JET).read().splitlines()]


def load_columns():
    """the committed file's numbers: dict z, u, v, w, T, rho, p"""
    a = np.array([[float(t) for t in row] for row in _tokens()])
    return dict(zip(("z", "u", "v", "w", "T", "rho", "p"), a.T))


def write_twin(path):
    """the committed file's very tokens in `zTuvdp` order (z, T, u, v, rho, p)"""
    with open(path, "w") as fh:
        for z, u, v, w, T, rho, p in _tokens():
            fh.write(" ".join([z, T, u, v, rho, p]) + "\n")
    return path


def write_toy_on_jet_nodes(path):
    """a second member for an ensemble with the jet (members share their nodes): ToyAtmo's own winds on the jet's nodes, T, rho, p and the z tokens of
    the committed file, in `zuvwTdp` order"""
    raw = np.loadtxt(H.TOYATMO)
    zs = load_columns()["z"]
    u0, v0 = np.interp(zs, raw[:, 0], raw[:, 2]), np.interp(zs, raw[:, 0], raw[:, 3])
    with open(path, "w") as fh:
        for (z, u, v, w, T, rho, p), a, b in zip(_tokens(), u0, v0):
            fh.write(" ".join([z, f"{a:.12g}", f"{b:.12g}", "0", T, rho, p]) + "\n")
    return path


def resampled(n):
    """z, T, u, v, rho of the jet linearly resampled on n even nodes (a profile too long for the kernels' LDS table when n > 1463)"""
    c = load_columns()
    z = np.linspace(0.0, c["z"][-1], n)
    return (z,) + tuple(np.interp(z, c["z"], c[k]) for k in ("T", "u", "v", "rho"))


# ---- tests/golden/jet_small.npz (make_golden.py `jet`): what its tables were made with, and how to read them ----
FIXTURE = os.path.join(H.GOLDEN_DIR, "jet_small.npz")
ESIZE = {H.EQ_GLOBAL: (6, 18), H.EQ_3D: (4, 12), H.EQ_2D: (3, 6)}          # state length without / with amplitudes
HIDX = {H.EQ_GLOBAL: None, H.EQ_3D: 2, H.EQ_2D: 1}                         # the height component compare_records judges against the turning height
# table -> (fan, parameters besides src and range_limit); fan a: ground source, fan b: source at SRC_Z, rays below the horizontal included
TABLES = {"a_amp1": ("a", dict(bounces=2, calc_amp=1)), "a_amp0": ("a", dict(bounces=2, calc_amp=0)),
          "b_amp1": ("b", dict(bounces=2, calc_amp=1)), "b_amp0": ("b", dict(bounces=2, calc_amp=0)),
          "b_zg": ("b", dict(bounces=2, calc_amp=1, z_grnd=0.3, freq=10.0, tweak_abs=0.6)),
          "b_f001": ("b", dict(bounces=2, calc_amp=1, freq=0.01))}


def src(eq, z):
    """the source at height z in the set's own layout (harness.make_cfg, Params.src)"""
    return {H.EQ_GLOBAL: (z, 30.0, 0.0), H.EQ_3D: (0.0, 0.0, z), H.EQ_2D: (z, 0.0, 0.0)}[eq]


def fan(g, tag):
    """theta, phi, source height of a table's fan"""
    name = TABLES[tag][0]
    return g[f"{name}_theta"], g[f"{name}_phi"], (float(g["src_z"]) if name == "b" else 0.0)


def table(g, eq, tag):
    """(records, step total, sens) of a table.  b_f001 is stored as its ATTEN column: the generator asserted every other column equal to b_amp1's"""
    key = f"{H.EQ_NAMES[eq]}_{tag}"
    if f"{key}_rec" in g.files:
        rec = g[f"{key}_rec"]
    else:
        rec = g[f"{H.EQ_NAMES[eq]}_b_amp1_rec"].copy()
        rec[..., H.REC["ATTEN"]] = g[f"{key}_atten"]
    return rec, int(g[f"{key}_steps"]), g[f"{key}_sens"]


def atmo(g, eq, key):
    """a probe / spline-table array of the set: the Cartesian sets share theirs (`cart_`), and no set changes T or rho on loading"""
    k = f"global_{key}" if eq == H.EQ_GLOBAL else f"cart_{key}"
    return g[k] if k in g.files else g[f"cart_{key}"]


if __name__ == "__main__":
    print(write_met(), os.path.getsize(JET), "bytes")
