"""Diagnostic: where one PCG workgroup spends an iteration (needs libvisfs_ba_hip_stamps.so built with -DVISFS_BA_STAMPS).
usage: python tools/pcg_stamps.py C2 [stamp library]
gate = head of the kernel to the test of the LM state, set-up = from there to the first iteration, tail = behind the last iteration to
the kernel's last store (x, the pose update, the statistics)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from visfs_amd import abi, backend, synth
backend.LIB_PATH = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "visfs_amd", "lib", "libvisfs_ba_hip_stamps.so")
lib = backend.load_library()
CFG = sys.argv[1] if len(sys.argv) > 1 else "C2"
for wg in (0, 24, 48):
    os.environ["VISFS_BA_STAMP_WG"] = str(wg)
    w = synth.make_window(CFG); prm = abi.default_params(iterations=20, solver=2)
    gb, *_ = abi.pack_window_with(lib.visfs_ba_pack_window, prm, abi.WindowBuffers(w))
    s = backend.Solver(prm); s.upload(gb)
    for _ in range(3):
        s.reset(); s.optimize()
    out = np.zeros(128)
    s.lib.visfs_ba_stage_fetch(s.h, 100, out.ctypes.data_as(C.POINTER(C.c_double)), 128)
    st = out.view(np.uint64)
    t_start = int(st[127]); t0 = int(st[0])
    t_head = int(st[126])
    gate = f"gate {(t_start - t_head) * 10} ns | " if 0 < t_head <= t_start else ""        # (slot 126: k_pcg1 of a lone window)
    print(f"wg {wg}: {gate}set-up {(t0 - t_start) * 10} ns")
    k = 0
    n_it = int(st[97]) if 0 < int(st[97]) <= 24 and int(st[98]) > t0 else 24      # (slots 97-99: k_pcg1 of a lone window; the slots from 32 on are also k_backsub's: an eighth iteration's last stamp is not its own)
    while k < n_it and 4 + 4 * k < 100 and st[4 + 4 * k] > st[0] and (k == 0 or st[4 + 4 * k] > st[4 * k]):
        a, b, c, d = (int(st[1 + 4 * k]), int(st[2 + 4 * k]), int(st[3 + 4 * k]), int(st[4 + 4 * k]))
        prev = t0 if k == 0 else int(st[4 * k])
        print(f"   iter {k}: matvec+barrier {(a - prev) * 10:6d} ns | publish {(b - a) * 10:5d} | gather+barrier {(c - b) * 10:6d} (extra sweeps {int(st[100 + k]) if k < 26 else -1}) | vector+barrier {(d - c) * 10:6d} | total {(d - prev) * 10}")
        k += 1
    if int(st[98]) > int(st[99]) > t0:
        print(f"   tail (the loop's exit to the last store: x, the pose update, the statistics) {(int(st[98]) - int(st[99])) * 10} ns | {int(st[97])} iterations | whole kernel {(int(st[98]) - (t_head or t_start)) * 10} ns")
    s.close()
