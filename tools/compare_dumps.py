#!/usr/bin/env python3
"""Bit-for-bit comparison of two `bench.py --dump-outputs` directories: every .npy of the first must exist in the second and be
numpy.array_equal (NaNs in the same places).  usage: tools/compare_dumps.py DIR_A DIR_B [label]; exit code 1 on any difference."""
import os, sys
import numpy as np
a, b = sys.argv[1], sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else f"{a} vs {b}"
names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
bad = 0
for f in names:
    if not os.path.exists(os.path.join(b, f)):
        print(f"{label}: {f} MISSING in {b}"); bad += 1; continue
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
    print(f"{label}: {f} {x.dtype}{list(x.shape)} {'identical' if same else 'DIFFERENT'}")
    bad += 0 if same else 1
if not names:
    print(f"{label}: no .npy in {a}"); bad = 1
print(f"{label}: {len(names)} arrays, {bad} differ")
sys.exit(1 if bad else 0)
