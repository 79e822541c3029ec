"""Diagnostic: timeline of one block's wave in k_schur_finalize_head (needs a library built with -DVISFS_BA_STAMPS: tools/build_stamps.sh;
VISFS_BA_KERNEL_FLAGS="-mllvm -amdgpu-kernarg-preload-count=8 -DVISFS_BA_CHAINS=0" builds the form without load windows).
usage: python tools/schur_stamps.py C2 [stamp library] [block ...]
Slots 110..115 of the stamp buffer: entry, gate passed, gather partials summed, all sums done (a diagonal block: pose-major partials and
odometry entries; an off-diagonal one: odometry entries), last store issued (behind the 6x6 inverse of a diagonal block), stores drained.
Shares, not run times: the stamps' own stores and waits are in the way."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from visfs_amd import abi, backend, synth
backend.LIB_PATH = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "visfs_amd", "lib", "libvisfs_ba_hip_stamps.so")
lib = backend.load_library()
CFG = sys.argv[1] if len(sys.argv) > 1 else "C2"
blocks = [int(x) for x in sys.argv[3:]] or [0, 1, 100, 200, 300]
names = ["head + gate", "gather partials (first wait + adds)", "pose-major / odometry sums", "inverse + stores issued", "stores drained"]
for b in blocks:
    os.environ["VISFS_BA_STAMP_WG"] = str(b)
    w = synth.make_window(CFG); prm = abi.default_params(iterations=20, solver=2)
    gb, *_ = abi.pack_window_with(lib.visfs_ba_pack_window, prm, abi.WindowBuffers(w))
    s = backend.Solver(prm); s.upload(gb)
    rows = []
    for _ in range(3):
        s.reset(); s.optimize()
        out = np.zeros(128)
        s.lib.visfs_ba_stage_fetch(s.h, 100, out.ctypes.data_as(C.POINTER(C.c_double)), 128)
        rows.append(out.view(np.uint64).astype(np.int64)[110:116].copy())
    t = rows[-1]
    if t[0] == 0 or np.any(np.diff(t) < 0):
        print(f"{CFG} block {b}: no complete set of stamps ({t.tolist()})")
    else:
        print(f"{CFG} block {b}: " + " | ".join(f"{names[i]} {(t[i + 1] - t[i]) * 10} ns" for i in range(5)) + f" | total {(t[5] - t[0]) * 10} ns"
              + " | totals of the three solves " + " ".join(str((r[5] - r[0]) * 10) for r in rows))
    s.close()
