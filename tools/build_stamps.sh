#!/bin/bash
# Diagnostic build of the HIP library with in-kernel real-time stamps (-DVISFS_BA_STAMPS): visfs_amd/lib/libvisfs_ba_hip_stamps.so.
# Never quote run times of this build; read the SHARES of its stamps (tools/pcg_stamps.py, tools/small_solve_stamps.py).
# ba_kernels.hip gets the product's kernel-argument preload flag (visfs_amd/build.py, KERNEL_FLAGS), in a compile step of its own.
# VISFS_BA_SRC=<dir> / VISFS_BA_KERNEL_FLAGS= / STAMPS_NAME=<name>: another checkout's sources, built without the flag, under another name.
set -e
cd "$(dirname "$0")/.."
src=${VISFS_BA_SRC:-visfs_amd/csrc}
kflags=${VISFS_BA_KERNEL_FLAGS--mllvm -amdgpu-kernarg-preload-count=8}
name=${STAMPS_NAME:-stamps}
mkdir -p build/obj visfs_amd/lib
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DVISFS_BA_STAMPS $kflags -c $src/ba_kernels.hip -o build/obj/ba_kernels_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DVISFS_BA_STAMPS -o visfs_amd/lib/libvisfs_ba_hip_$name.so build/obj/ba_kernels_$name.o $src/ba_cov.hip $src/ba_submap.hip $src/ba_api.cpp -lpthread
