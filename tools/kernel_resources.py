#!/usr/bin/env python3
"""Register / scratch / occupancy table of every kernel in ba_kernels.hip, ba_cov.hip, ba_flow.hip, ba_corners.hip, ba_pnp.hip, ba_fund.hip, ba_clahe.hip, ba_tracker.hip, ba_scan.hip, ba_scan_fast.hip, ba_scan_group.hip, ba_scan_refine.hip, ba_pose_graph.hip, ba_pose_graph_cov.hip, ba_map.hip, ba_scan_filter.hip, ba_mcl.hip, ba_mcl_kld.hip, ba_place.hip and ba_place_verify.hip (hipcc -Rpass-analysis=kernel-resource-usage,
device only).
usage: tools/kernel_resources.py [filter-substring ...]   (extra -D flags through VISFS_BA_EXTRA_FLAGS; KRES_TXT=<file> reuses a saved remark dump;
VISFS_BA_SRC=<dir>: another checkout's visfs_amd/csrc)"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfs_amd.build import KERNEL_FLAGS, KERNEL_SOURCES
srcs = [os.path.join(os.environ.get("VISFS_BA_SRC", os.path.join(ROOT, "visfs_amd", "csrc")), f) for f in ("ba_kernels.hip", "ba_cov.hip", "ba_flow.hip", "ba_corners.hip", "ba_pnp.hip", "ba_fund.hip", "ba_clahe.hip", "ba_tracker.hip", "ba_scan.hip", "ba_scan_fast.hip", "ba_scan_group.hip", "ba_scan_refine.hip", "ba_pose_graph.hip", "ba_pose_graph_cov.hip", "ba_map.hip", "ba_scan_filter.hip", "ba_mcl.hip", "ba_mcl_kld.hip", "ba_place.hip", "ba_place_verify.hip")]
if os.environ.get("KRES_TXT"):
    txt = open(os.environ["KRES_TXT"]).read()
else:
    txt = ""
    for src in srcs:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", "/tmp/_kres.o"]
        cmd += os.environ.get("VISFS_BA_EXTRA_FLAGS", "").split()
        if os.path.basename(src) in KERNEL_SOURCES and not os.environ.get("KRES_NO_PRELOAD"):      # (as the product compiles it; KRES_NO_PRELOAD=1: as the commits before the head arguments did)
            cmd += KERNEL_FLAGS
        txt += subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in txt.splitlines():
    m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\S+) \[-Rpass", line)
    if not m: continue
    key, val = m.group(1).strip(), m.group(2)
    if key == "Function Name":
        cur = {"name": val}; rows.append(cur)
    elif cur is not None and val.lstrip("-").isdigit():
        cur[key] = int(val)
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
flt = sys.argv[1:]
print(f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'spillV':>6} {'scratch':>7} {'occ':>3} {'LDS':>6}  kernel")
for r, n in zip(rows, names):
    name = re.sub(r"\(.*\)$", "", n.replace("visfs_ba::", "").replace("void ", ""))
    if flt and not all(f in name for f in flt): continue
    print(f"{r.get('VGPRs', -1):>5} {r.get('AGPRs', -1):>5} {r.get('TotalSGPRs', -1):>5} {r.get('VGPRs Spill', -1):>6} {r.get('ScratchSize [bytes/lane]', -1):>7} {r.get('Occupancy [waves/SIMD]', -1):>3} {r.get('LDS Size [bytes/block]', -1):>6}  {name}")
