#!/bin/bash
# A/B measurement build of the HIP library with extra -D flags: tools/build_variant.sh <name> -DVISFS_BA_TILE_N=0 ...
# -> visfs_amd/lib/libvisfs_ba_hip_<name>.so; select it with VISFS_BA_LIB=<path> (visfs_amd/backend.py).
# VISFS_BA_SRC=<dir> builds the sources of another checkout's visfs_amd/csrc instead (the parent commit's library for an A/B:
#   git archive <commit> visfs_amd/csrc include | tar -x -C <dir>; VISFS_BA_SRC=<dir>/visfs_amd/csrc tools/build_variant.sh parent).
# ba_kernels.hip is compiled on its own with the product's kernel-argument preload flag (visfs_amd/build.py, KERNEL_FLAGS);
# VISFS_BA_KERNEL_FLAGS= (empty) builds it without, as the commits before the head arguments were built.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
src=${VISFS_BA_SRC:-visfs_amd/csrc}
kflags=${VISFS_BA_KERNEL_FLAGS--mllvm -amdgpu-kernarg-preload-count=8}
files=""
for f in ba_cov.hip ba_submap.hip ba_flow.hip ba_corners.hip ba_clahe.hip ba_pnp.hip ba_fund.hip ba_tracker.hip ba_scan.hip ba_scan_fast.hip ba_api.cpp ba_scan_group.hip ba_scan_refine.hip ba_pose_graph.hip ba_pose_graph_cov.hip ba_map.hip ba_scan_filter.hip; do
  [ -f "$src/$f" ] && files="$files $src/$f"
done
mkdir -p build/obj visfs_amd/lib
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $kflags "$@" -c $src/ba_kernels.hip -o build/obj/ba_kernels_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared "$@" -o visfs_amd/lib/libvisfs_ba_hip_$name.so build/obj/ba_kernels_$name.o $files -lpthread
