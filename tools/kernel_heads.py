#!/usr/bin/env python3
"""Head report of every kernel in ba_kernels.hip: how many serial scalar round trips precede the first vector-memory
instruction.  Compiles the file device-only to assembly (as tools/kernel_resources.py compiles it, with the product's kernel-argument
preload flag) and prints per kernel
  preload  the descriptor's .amdhsa_user_sgpr_kernarg_preload_length (dwords of kernel arguments that arrive in user SGPRs),
  waits    s_waitcnt on outstanding scalar loads between the entry and the first vector-memory instruction, in text order,
  karg     ... of which wait for a load from the kernel-argument segment: the cold round trips the head arguments remove.
With a non-zero preload length the count starts behind the 256-byte compatibility prologue (one s_load of the same dwords for
firmware that does not preload), at the entry the hardware really uses.
usage: tools/kernel_heads.py [filter-substring ...]   (KHEADS_S=<file> reuses a saved .s; VISFS_BA_SRC=<dir> reads another checkout's
visfs_amd/csrc; VISFS_BA_EXTRA_FLAGS adds flags; KHEADS_NO_PRELOAD=1 compiles without the preload flag: the parent's build)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.environ.get("VISFS_BA_SRC", os.path.join(ROOT, "visfs_amd", "csrc"))


def assembly():
    if os.environ.get("KHEADS_S"):
        return open(os.environ["KHEADS_S"]).read()
    flags = []
    if not os.environ.get("KHEADS_NO_PRELOAD"):
        from visfs_amd.build import KERNEL_FLAGS
        flags = list(KERNEL_FLAGS)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ba_kernels.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"] + flags
        cmd += os.environ.get("VISFS_BA_EXTRA_FLAGS", "").split() + [os.path.join(SRC, "ba_kernels.hip"), "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(res.stderr)
        return open(out).read()


VMEM = re.compile(r"^(global_|buffer_|flat_|scratch_|tbuffer_)")
SLOAD = re.compile(r"^s_(?:buffer_)?load_\w+\s+(s\[\d+:\d+\]|s\d+),\s*(s\[(\d+):(\d+)\])")


def user_sgpr_of_kernarg(desc):
    """Index of the first SGPR of the kernel-argument segment pointer: the user SGPRs are dealt in a fixed order."""
    n = 0
    for key, width in (("private_segment_buffer", 4), ("dispatch_ptr", 2), ("queue_ptr", 2)):
        if desc.get("user_sgpr_" + key, 0):
            n += width
    return n


def head_of(lines, preload, karg0):
    """(scalar waits, of which on kernel-argument loads, instructions) in front of the first vector-memory instruction."""
    i = 0
    if preload:
        # compatibility prologue: s_load of the preloaded dwords, wait, branch over the padding to the aligned real entry
        for k, ln in enumerate(lines):
            if ln.startswith(".p2align") and "8" in ln:
                i = k + 1
                break
    karg = {karg0}                    # first registers of the pairs that hold the segment pointer (copies included)
    pending, pending_karg, waits, waits_karg, n = 0, 0, 0, 0, 0
    for ln in lines[i:]:
        if not ln or ln.startswith((";", ".")) or ln.endswith(":"):
            continue
        n += 1
        op = ln.split()[0]
        if VMEM.match(op):
            return waits, waits_karg, n - 1
        m = re.match(r"^s_mov_b64\s+s\[(\d+):\d+\],\s*s\[(\d+):\d+\]", ln)
        if m and int(m.group(2)) in karg:
            karg.add(int(m.group(1)))
        m = SLOAD.match(ln)
        if m:
            pending += 1
            if int(m.group(3)) in karg:
                pending_karg += 1
            continue
        if op == "s_waitcnt" and ("lgkmcnt(0)" in ln or re.match(r"^s_waitcnt\s+(0x0|0)\s*$", ln)):
            if pending:
                waits += 1
                if pending_karg:
                    waits_karg += 1
            pending = pending_karg = 0
    return waits, waits_karg, n


def main():
    txt = assembly()
    kernels = {}
    # kernel bodies: "<symbol>:" ... "s_endpgm"; descriptors: ".amdhsa_kernel <symbol>" ... ".end_amdhsa_kernel"
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.S | re.M):
        desc = {k: int(v, 0) for k, v in re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)) if re.match(r"^(0x)?[0-9a-fA-F]+$", v)}
        kernels[m.group(1)] = desc
    rows = []
    for sym, desc in kernels.items():
        m = re.search(r"^" + re.escape(sym) + r":.*?\n(.*?)^\s*s_endpgm", txt, re.S | re.M)
        if not m:
            continue
        lines = [ln.strip() for ln in m.group(1).splitlines()]
        preload = desc.get("user_sgpr_kernarg_preload_length", 0)
        rows.append((sym, preload) + head_of(lines, preload, user_sgpr_of_kernarg(desc)))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
    flt = sys.argv[1:]
    print(f"{'preload':>7} {'waits':>5} {'karg':>4} {'instr':>5}  kernel")
    for r, n in zip(rows, names):
        name = re.sub(r"\(.*\)$", "", n.replace("visfs_ba::", "").replace("void ", ""))
        if flt and not all(f in name for f in flt):
            continue
        print(f"{r[1]:>7} {r[2]:>5} {r[3]:>4} {r[4]:>5}  {name}")


if __name__ == "__main__":
    main()
