"""The owner types of the shared host layer (visfs_amd/csrc/ba_host.hpp: DeviceBuf, PinnedBuf, Staged, Event) without a GPU and
without the HIP runtime: tests/cpp/host_owner_test.cpp, a stand-alone program compiled with plain g++ that defines the runtime entry
points the owners call itself (malloc/free, a table of live blocks, a switch that fails the k-th call).  It checks that a block is
freed once, that a move and a failed release leave an owner empty, the growth rule, that a grow or a paired reserve whose k-th
runtime call fails leaves nothing alive, nothing freed twice and capacity 0 beside a null pointer, and the three shapes that went
wrong with raw pointers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_owner(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    exe = tmp_path / "host_owner_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "host_owner_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr
