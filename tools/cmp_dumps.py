"""Bitwise comparison of the .npy arrays of two directories (bench.py --dump-outputs DIR, tools/dump_small_fans.py DIR), as uint64 words.
usage: cmp_dumps.py DIR_A DIR_B   (exit status 1 if any array differs or is missing)"""
import os, sys
import numpy as np
a_dir, b_dir = sys.argv[1], sys.argv[2]
names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
ok = bool(names) and names == sorted(f for f in os.listdir(b_dir) if f.endswith(".npy"))
for f in names:
    a = np.load(os.path.join(a_dir, f))
    b = np.load(os.path.join(b_dir, f)) if os.path.exists(os.path.join(b_dir, f)) else None
    same = b is not None and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    ok &= same
    print(f"{f}: shape {a.shape} {a.dtype}: " + ("bit-identical" if same else "DIFFERENT"))
print("RESULT: " + ("all bit-identical" if ok else "NOT identical"))
sys.exit(0 if ok else 1)
