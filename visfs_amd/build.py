"""Build helper: hipcc for the gfx950 library (the test-side checker under oracle/ has its own Makefile)."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visfs_amd", "csrc")
LIB_DIR = os.path.join(ROOT, "visfs_amd", "lib")
LIB = os.path.join(LIB_DIR, "libvisfs_ba_hip.so")
SOURCES = ["ba_kernels.hip", "ba_cov.hip", "ba_submap.hip", "ba_flow.hip", "ba_corners.hip", "ba_clahe.hip", "ba_pnp.hip", "ba_fund.hip", "ba_tracker.hip", "ba_scan.hip", "ba_scan_fast.hip", "ba_api.cpp", "ba_scan_group.hip", "ba_scan_refine.hip", "ba_pose_graph.hip", "ba_pose_graph_cov.hip", "ba_map.hip", "ba_scan_filter.hip", "ba_mcl.hip", "ba_mcl_kld.hip", "ba_place.hip", "ba_place_verify.hip"]
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(ROOT, "include", "*.h")))      # every header: a new one cannot be forgotten


# ba_kernels.hip alone is compiled with kernel-argument preloading: the leading scalar parameters of its k_*_head kernels
# (at most eight of them, 14 dwords) arrive in user SGPRs at wave launch.  A by-value struct is never preloaded, so every other kernel
# of the file compiles as without the flag; the other sources do not get it at all.
KERNEL_FLAGS = ["-mllvm", "-amdgpu-kernarg-preload-count=8"]
KERNEL_SOURCES = ["ba_kernels.hip"]
KERNEL_OBJ_DIR = os.path.join(ROOT, "build", "obj")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_hip(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 → visfs_amd/lib/libvisfs_ba_hip.so (in-tree, travels with gpurun)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + HEADERS
    if not force and not _stale(LIB, deps):
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(LIB_DIR, exist_ok=True)
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    os.makedirs(KERNEL_OBJ_DIR, exist_ok=True)
    objs = [os.path.join(KERNEL_OBJ_DIR, os.path.splitext(k)[0] + ".o") for k in KERNEL_SOURCES]
    cmds = [common + KERNEL_FLAGS + ["-c", os.path.join(CSRC, k), "-o", o] for k, o in zip(KERNEL_SOURCES, objs)]     # a compile step of its own
    cmds.append(common + ["-shared", "-o", LIB] + objs + [x for x in srcs if os.path.basename(x) not in KERNEL_SOURCES] + ["-lpthread"])
    for cmd in cmds:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)     # a normal build takes a few minutes
        if verbose or res.returncode != 0:
            print(" ".join(cmd)); print(res.stdout); print(res.stderr)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + res.stderr)
    return LIB



HOST = os.path.join(ROOT, "visfs_amd", "host")
WINDOW_LIB = os.path.join(LIB_DIR, "libvisfs_window.so")
WINDOW_SOURCES = ["WindowMap.cpp", "window_capi.cpp"]


def build_host(force=False, verbose=False):
    """g++ → visfs_amd/lib/libvisfs_window.so: the host-side sliding-window container (include/visfs_window.h), no GPU code."""
    srcs = [os.path.join(HOST, s) for s in WINDOW_SOURCES]
    deps = srcs + [os.path.join(HOST, "WindowMap.h"), os.path.join(ROOT, "include", "visfs_window.h"), os.path.join(ROOT, "include", "visfs_ba.h")]
    if not force and not _stale(WINDOW_LIB, deps):
        return WINDOW_LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", WINDOW_LIB] + srcs
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd)); print(res.stdout); print(res.stderr)
    if res.returncode != 0:
        raise RuntimeError("g++ failed:\n" + res.stderr)
    return WINDOW_LIB
