"""The shared host layer of the GPU objects (visfs_amd/csrc/ba_host.hpp) without a GPU: tests/cpp/host_guard_test.cpp, a stand-alone
program compiled with plain g++ and linked against the HIP runtime for hipGetErrorString only — no call in it needs a device.  It
checks the text and the return of a failed and of a passing HIP check on every kind of sink, the C ABI's exception guard for every
kind of exception (null sinks included), and the helpers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_guard(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    exe = tmp_path / "host_guard_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "host_guard_test.cpp"),
                    "-L" + os.path.join(rocm, "lib"), "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lamdhip64", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr
