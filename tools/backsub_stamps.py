"""Diagnostic: timeline of one landmark workgroup of the fused speculative kernel k_backsub<LINA> (needs libvisfs_ba_hip_stamps.so built
with -DVISFS_BA_STAMPS: tools/build_stamps.sh).  usage: python tools/backsub_stamps.py C2 [stamp library]
"gate" runs from the head of the kernel to the test of the LM state: in the lone-window form it covers everything that is loaded in front of
that test (both estimate buffers, the landmark's index data, the lane's first observation)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from visfs_amd import abi, backend, synth
backend.LIB_PATH = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "visfs_amd", "lib", "libvisfs_ba_hip_stamps.so")
lib = backend.load_library()
CFG = sys.argv[1] if len(sys.argv) > 1 else "C2"
for wg in (0, 100, 300):
    os.environ["VISFS_BA_STAMP_WG"] = str(wg)
    w = synth.make_window(CFG); prm = abi.default_params(iterations=20, solver=2)
    gb, *_ = abi.pack_window_with(lib.visfs_ba_pack_window, prm, abi.WindowBuffers(w))
    s = backend.Solver(prm); s.upload(gb)
    for _ in range(3):
        s.reset(); s.optimize()
    out = np.zeros(128)
    s.lib.visfs_ba_stage_fetch(s.h, 100, out.ctypes.data_as(C.POINTER(C.c_double)), 128)
    t = out.view(np.uint64).astype(np.int64)[32:39]
    names = ["gate (LmState)", "pose staging + barrier", "back-substitution + trial chi2", "two block sums", "role A of the linearisation"]
    line = " | ".join(f"{names[i]} {(t[i + 1] - t[i]) * 10} ns" for i in range(5))
    if t[2] < t[6] < t[3]:                       # (a library older than this stamp leaves the slot to another kernel)
        line += f" | of the third: back-substitution {(t[6] - t[2]) * 10} ns, trial chi2 {(t[3] - t[6]) * 10} ns"
    print(f"{CFG} workgroup {wg}: " + line + f" | total {(t[5] - t[0]) * 10} ns")
    s.close()
