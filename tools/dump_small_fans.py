"""The records of the small golden fan of the stratified Global set (tests/golden/global_small.npz: 18 rays) as one array, for a bitwise A/B of two builds of
the library (GEOAC_LIB names the other one): CalcAmp on and off with two bounces, and the fixture's alternate configuration (source at 41.131 N).
usage: dump_small_fans.py DIR   -> DIR/small_fans.npy (4608 float64);  compare two directories with tools/cmp_dumps.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import geoac_amd as G
import harness as H
g = np.load(os.path.join(H.GOLDEN_DIR, "global_small.npz"))
out = []
for params in (dict(bounces=2, calc_amp=1, mode=0), dict(bounces=2, calc_amp=0, mode=0),
               dict(bounces=1, calc_amp=1, mode=0, src=(1.0, 41.131, -112.896), z_grnd=0.3, tweak_abs=0.5, freq=0.5, range_limit=800.0)):
    ctx = G.FanContext(G.EQ_GLOBAL, device=0); ctx.load_met(H.TOYATMO); ctx.set_params(**params)
    rec, steps = ctx.run(g["theta"], g["phi"])
    out.append(np.asarray(rec, dtype=np.float64).ravel().copy()); ctx.close()
os.makedirs(sys.argv[1], exist_ok=True)
np.save(os.path.join(sys.argv[1], "small_fans.npy"), np.concatenate(out))
print("library", G.library_path(), "->", os.path.join(sys.argv[1], "small_fans.npy"), sum(len(a) for a in out), "values")
